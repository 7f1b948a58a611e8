// ow_schedule.h -- what crosses between the two host units behind the frame entry points: ow_schedule.hip (the tick scheduler: which launches
// a call turns into) and ow_runtime.hip (the context's housekeeping).  main_stream, sync_stream, refuse_faulted and check_cascade, which the
// read side needs too, are declared in ow_context.h.
#pragma once
#include "ow_context.h"

namespace ow {
// ---- ow_schedule.hip, for ow_create ----
// the merged launch shapes this context will use (batch sizes, tick-group depth, pair slots), and the forms pinned by `flags`
void plan_tick_groups(ow_context *c, uint32_t flags);
// launch slots of scratch intermediate: what one batch needs, and the most the look-ahead of ow_update_all / ow_process can ever ask for
int base_scratch_slots(const ow_context *c);
int lookahead_scratch_slots(const ow_context *c);
// ---- ow_schedule.hip, for whatever else writes the scratch, may have corrupted it, or changes what it was computed from ----
// drops the work computed ahead: the look-ahead queue and a run's work-ahead for the next run
void drop_computed_ahead(ow_context *c);
// ---- ow_runtime.hip, for the scheduler ----
// at least `slots` launch slots of scratch intermediate (grows by replacing it: synchronises, and drops the work computed ahead)
ow_status ensure_scratch(ow_context *c, int slots);
// the next four events of the timing pool (single: the record times ONE launch, events 0 and 1 -- a tick group / pair)
ow_status next_events(ow_context *c, hipEvent_t **out, bool single = false);
}  // namespace ow
