// ow_spray.h -- the sea-spray particle emitter (sea_spray_particle.gdshader, the scene's WaterSprayEmitter): the engine's restart
// schedule, the shader's start() :45-66 and process() :74-126 for one particle, the records, and the host's clock.
//
// Compiles as device code (ow_spray.hip, built with -ffp-contract=off) and as plain C++ (tests/spray/, g++ -ffp-contract=off), like
// ow_surface.h: every FP32 operation is an IEEE-754 add, multiply, divide or square root, a floor, a conversion or a compare; exp and log
// are exp_f32 (ow_surface.h) and log_f32 (ow_shading.h), written out in those operations.  There is no library transcendental, so both builds
// produce the same bits for every input.
//
// WHAT THE SHADER TEXT DOES NOT CONTAIN, AS DECIDED HERE
//   clock     The host holds `time` in FP64.  A step sets time_new = time + delta, TIME = (float)time_new, uint(TIME) a host-computed
//             uint32, cycle = floor(time_new / L) with L = emitter_lifetime, phase = (float)(fmod(time_new, L) / L); prev is the previous
//             step's phase (0 at creation); wrapped = cycle > the previous cycle, decided in FP64.
//   restart   The engine's schedule at explosiveness 0 and randomness 0, no fixed FPS, no interpolation: rp = (float)i / (float)amount,
//             particle i restarts iff wrapped ? (rp >= prev || rp < phase) : (rp >= prev && rp < phase).  NUMBER = (uint32)(cycle amount
//             + i), minus amount when wrapped && rp >= prev, modulo 2^32.  A particle is not ACTIVE before its first restart.
//   start()   ACTIVE = true; hash32 as written on p = (NUMBER + uint(TIME) + seed, 1 + uint(TIME) + seed); uint -> float rounds to
//             nearest and float(0x7FFFFFFF) is 2^31, so a component may be exactly 1.  t = (uint32)sqrtf((float)num_particles) comes from
//             the host.  coords is :52 as written; START_POS_r = (E_r0 cx + E_r2 cz) + E_r3; CUSTOM.z, PARTICLE_LIFETIME and START_TIME are
//             :56-59 as written with LIFETIME = L; HAS_STARTED = 0; position (0, -1e10, 0); scale 1e-3 on the three axes; CUSTOM.w = 0
//             (the engine clears CUSTOM on a restart).
//   G1        The shader's set_scale re-normalises the columns it stored last step, and :122-123 store a zero column whenever t = 0
//             (exp_impulse(0) = 0, log(1) = 0): the next normalize is 0/0.  Here the three unit axes are the emission basis' columns,
//             normalised once on the host in FP64 and narrowed, and every set_scale is axis_k * scale_k: the shader's value wherever the
//             shader is defined (up to the rounding of a repeated normalize), and never NaN.
//   process() runs in the same step as a restart and not at all for a particle that is not ACTIVE.  The branches run in the shader's
//             order on FP32 values compared as written; START_TIME + PARTICLE_LIFETIME is one FP32 add.  The spawn decision :80-89 and the
//             displacement sum :105-109 are sample_point's (ow_surface.h) at START_POS.xz: k_sample_surface's call, so its bits.  :92-95,
//             :99-100, :112-116 and :119-124 are as written with exp -> exp_f32, log(1 + t) -> log_f32(1.0f + t), pow(x, 2.0) -> x x, and
//             PARTICLE_LIFETIME / lifetime an FP32 division.
//   G2        Finite maps give finite records.  Where a map texel is not finite and a result is not, the particle's instance is written
//             as zeros, its ACTIVE flag is lowered and it leaves the draw list; its stored scale and scale_factor are zeroed.
//   instance  A particle that is not ACTIVE carries twelve zeros (the engine's copy pass) and custom = (0, 0, CUSTOM.z, 0).
//   draw list The indices of the particles that are ACTIVE and HAS_STARTED after the step, ascending; live_count is their number.
#pragma once

#include <cmath>

#include "ow_shading.h"

namespace ow {

// layout-identical to ow_spray_options / ow_spray_instance / ow_spray_particle in include/ocean_waves.h
struct SprayOptions {
    uint32_t amount, num_particles;
    float emitter_lifetime, lifetime, lifetime_randomness;
    float particle_scale[3];
    uint32_t random_seed, reserved0;
    float emission_transform[12];
    double start_time;
    uint32_t reserved[8];
};
struct SprayInstance {
    float row[3][4];  // rows 0..2 of the transform: three basis components, then the origin's
    float custom[4];  // (0, 0, CUSTOM.z, CUSTOM.w)
};
struct SprayParticle {
    float start_pos[3], start_time;
    float particle_scale[3], particle_lifetime;
    float custom_z, scale_factor;
    uint32_t flags, number;
};
static_assert(sizeof(SprayOptions) == 128 && sizeof(SprayInstance) == 64 && sizeof(SprayParticle) == 48, "record layout");

constexpr uint32_t kSprayActive = 1u, kSprayHasStarted = 2u, kSprayRestarted = 4u;
constexpr uint32_t kSprayMinAmount = 4u, kSprayMaxAmount = 1048576u;
constexpr int kSprayBlock = 256;       // lanes per block of both kernels
constexpr int kSprayBlockWords = 8;    // per-block words of a step: live count, the four waves' bases, spawned, rejected, 0
constexpr int kSprayMaxBlocks = (int)(kSprayMaxAmount / kSprayBlock);

// an emitter's constants, resolved once from the options
struct SprayParams {
    uint32_t amount, t, seed;
    float emitter_lifetime, lifetime, randomness;  // L, lifetime, lifetime_randomness
    float particle_scale[3];
    float E[3][4];     // EMISSION_TRANSFORM, rows
    float axis[3][3];  // axis[k][r]: component r of the k-th unit axis (G1)
};
// one step's clock
struct SprayClock {
    float time;       // TIME
    uint32_t utime;   // uint(TIME)
    float prev, phase;
    int32_t wrapped;
    uint32_t base;    // (uint32)(cycle amount), modulo 2^32
};
// the host's side of an emitter: the FP64 clock and its bookkeeping
struct SprayHostState {
    double time = 0.0, cycle = 0.0;
    float prev = 0.0f;
    uint64_t steps = 0, restarts = 0;
};

// ---- lane code ------------------------------------------------------------------------------------------------------------------------

// :31-37 as written; out[k] in [0, 1]
OW_DEV void hash32(uint32_t px, uint32_t py, float out[3]) {
    const uint32_t qx = 1103515245u * ((px >> 1) ^ py), qy = 1103515245u * ((py >> 1) ^ px);
    const uint32_t h32 = 1103515245u * (qx ^ (qy >> 3));
    const uint32_t n = h32 ^ (h32 >> 16);
    const uint32_t rz[3] = {n, n * 16807u, n * 48271u};
    const float denom = (float)0x7FFFFFFFu;  // 2^31
    for (int k = 0; k < 3; ++k) out[k] = (float)((rz[k] >> 1) & 0x7FFFFFFFu) / denom;
}

// :69-72
OW_DEV float exp_impulse(float x, float k) {
    const float h = k * x;
    return h * exp_f32(1.0f - h);
}

// the restart schedule: does particle i restart this step, and with which NUMBER
OW_DEV bool spray_restart(const SprayParams &P, const SprayClock &K, uint32_t i, uint32_t *number) {
    const float rp = (float)i / (float)P.amount;
    const bool late = rp >= K.prev, early = rp < K.phase;
    *number = K.base + i - ((K.wrapped && late) ? P.amount : 0u);
    return K.wrapped ? (late || early) : (late && early);
}

// :45-66: the state a restart leaves (the transform it leaves is spray_waiting's)
OW_DEV void spray_start(const SprayParams &P, const SprayClock &K, uint32_t i, uint32_t number, SprayParticle &s) {
    float rand[3];
    hash32(number + K.utime + P.seed, 1u + K.utime + P.seed, rand);
    const float ft = (float)P.t - 1.0f;
    const float cx = ((float)(i / P.t) / ft - 0.5f) * 10.0f, cz = ((float)(i % P.t) / ft - 0.5f) * 10.0f;
    for (int r = 0; r < 3; ++r) s.start_pos[r] = (P.E[r][0] * cx + P.E[r][2] * cz) + P.E[r][3];
    s.custom_z = rand[0];
    s.particle_lifetime = P.lifetime - P.lifetime * P.randomness * rand[1];
    s.start_time = K.time + rand[2] * (P.emitter_lifetime - s.particle_lifetime);
    s.particle_scale[0] = s.particle_scale[1] = s.particle_scale[2] = 0.0f;
    s.scale_factor = 0.0f;
    s.flags = kSprayActive | kSprayRestarted;
    s.number = number;
}

OW_DEV void spray_instance_zero(const SprayParticle &s, SprayInstance &o) {
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) o.row[r][k] = 0.0f;
    o.custom[0] = o.custom[1] = o.custom[3] = 0.0f;
    o.custom[2] = s.custom_z;
}
// set_scale (G1) and the origin
OW_DEV void spray_instance_set(const SprayParams &P, const float scale[3], const float pos[3], float custom_w, const SprayParticle &s,
                               SprayInstance &o) {
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) o.row[r][k] = P.axis[k][r] * scale[k];
        o.row[r][3] = pos[r];
    }
    o.custom[0] = o.custom[1] = 0.0f;
    o.custom[2] = s.custom_z;
    o.custom[3] = custom_w;
}
OW_DEV bool spray_finite(float v) { return fabsf(v) <= 3.4028235e38f; }

// :74-126 for a particle that is ACTIVE on entry: its state after the step and its instance.  spawn: 0, or :89's outcome where it ran
// (1 spawned, 2 rejected).  Returns whether the particle is in the draw list.
OW_DEV bool spray_process(const u16x4 *disp, const u16x4 *norm, int n, int cascades, const SurfaceScales &scales, const SprayParams &P,
                          const SprayClock &K, SprayParticle &s, SprayInstance &o, int *spawn) {
    *spawn = 0;
    if (K.time > s.start_time + s.particle_lifetime) {  // :75-76
        s.flags &= ~kSprayActive;
        spray_instance_zero(s, o);
        return false;
    }
    if (!(K.time >= s.start_time)) {  // before :77: what start() left
        const float scale[3] = {1e-3f, 1e-3f, 1e-3f}, pos[3] = {0.0f, -1e10f, 0.0f};
        spray_instance_set(P, scale, pos, 0.0f, s, o);
        return false;
    }
    if (!(s.flags & kSprayHasStarted)) {  // :78-96
        const SurfaceSample m = sample_point(disp, norm, n, cascades, scales, s.start_pos[0], s.start_pos[2]);
        const bool active = m.spray_active != 0;
        s.scale_factor = m.scale_factor;
        const float base = m.foam_factor * ((active ? 1.0f : 0.0f) + 1e-3f);
        s.particle_scale[0] = base * 1.0f * P.particle_scale[0];
        s.particle_scale[1] = base * m.normal_factor * P.particle_scale[1];
        s.particle_scale[2] = base * 1.0f * P.particle_scale[2];
        s.flags = (s.flags & ~kSprayActive) | kSprayHasStarted | (active ? kSprayActive : 0u);
        *spawn = active ? 1 : 2;
    }
    if (!(s.flags & kSprayActive)) {
        spray_instance_zero(s, o);
        return false;
    }
    // :98-125
    const SurfaceSample m = sample_point(disp, norm, n, cascades, scales, s.start_pos[0], s.start_pos[2]);
    const float t = (K.time - s.start_time) / s.particle_lifetime;
    const float custom_w = exp_impulse(t, 10.0f);
    const float x = 2.5f * t - 0.45f;
    float d[3] = {m.displacement[0] * 0.75f, m.displacement[1] * 1.0f, m.displacement[2] * 0.75f};
    d[0] += 0.0f;
    d[1] += -5.0f * (x * x) * s.scale_factor + 0.5f;
    d[2] += 0.0f;
    const float pos[3] = {s.start_pos[0] + d[0], s.start_pos[1] + d[1], s.start_pos[2] + d[2]};
    const float size = s.particle_lifetime / P.lifetime;
    const float sm = size * size, lg = log_f32(1.0f + t);
    const float scale[3] = {s.particle_scale[0] * (sm * lg), s.particle_scale[1] * (sm * exp_impulse(t, 3.0f)), s.particle_scale[2] * (sm * lg)};
    spray_instance_set(P, scale, pos, custom_w, s, o);
    bool finite = spray_finite(custom_w);  // G2
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) finite = finite && spray_finite(o.row[r][k]);
    if (!finite) {
        s.flags &= ~kSprayActive;
        s.particle_scale[0] = s.particle_scale[1] = s.particle_scale[2] = 0.0f;
        s.scale_factor = 0.0f;
        spray_instance_zero(s, o);
        return false;
    }
    return true;
}

// One particle's step.  s: its state (read; rewritten where `wrote`), o: its instance (written where `wrote`: a particle that is not
// ACTIVE and does not restart keeps the zeros it has).  Returns whether it is in the draw list.
struct SprayLane {
    bool wrote, live, restarted;
    int spawn;
};
OW_DEV SprayLane spray_lane(const u16x4 *disp, const u16x4 *norm, int n, int cascades, const SurfaceScales &scales, const SprayParams &P,
                            const SprayClock &K, uint32_t i, SprayParticle &s, SprayInstance &o) {
    SprayLane out;
    uint32_t number;
    out.restarted = spray_restart(P, K, i, &number);
    out.spawn = 0;
    out.wrote = out.live = false;
    if (out.restarted) spray_start(P, K, i, number, s);
    if (!(s.flags & kSprayActive)) return out;  // dormant: nothing to run, nothing to write
    // still waiting for its start time: the state and the instance its restart left stand
    if (!out.restarted && !(K.time > s.start_time + s.particle_lifetime) && !(K.time >= s.start_time)) return out;
    out.wrote = true;
    out.live = spray_process(disp, norm, n, cascades, scales, P, K, s, o, &out.spawn);
    return out;
}

// ---- the host's side (plain host C++ in both builds) -----------------------------------------------------------------------------------

// mat_spray.tres and main.tscn:133-140: 32 768 particles, emitter lifetime 6 s, the 15 x emission transform at (-1, 0, -25)
inline void spray_default_options(SprayOptions *o) {
    __builtin_memset(o, 0, sizeof(*o));
    o->amount = 32768u;
    o->num_particles = 0u;
    o->emitter_lifetime = 6.0f;
    o->lifetime = 3.0f;
    o->lifetime_randomness = 0.25f;
    o->particle_scale[0] = 20.0f;
    o->particle_scale[1] = 8.5f;
    o->particle_scale[2] = 20.0f;
    o->emission_transform[0] = o->emission_transform[5] = o->emission_transform[10] = 15.0f;
    o->emission_transform[3] = -1.0f;
    o->emission_transform[7] = 0.0f;
    o->emission_transform[11] = -25.0f;
    o->start_time = 0.0;
}

// nullptr, or why ow_spray_create refuses these options; on success *P and *H are the emitter's constants and its clock at creation
inline const char *spray_resolve(const SprayOptions &o, SprayParams *P, SprayHostState *H) {
    if (o.amount < kSprayMinAmount || o.amount > kSprayMaxAmount) return "amount outside [4, 1048576]";
    const float scalars[] = {o.emitter_lifetime, o.lifetime, o.lifetime_randomness, o.particle_scale[0], o.particle_scale[1], o.particle_scale[2]};
    for (float v : scalars)
        if (!std::isfinite(v)) return "a value is not finite";
    for (float v : o.emission_transform)
        if (!std::isfinite(v)) return "emission_transform is not finite";
    if (!std::isfinite(o.start_time)) return "start_time is not finite";
    if (!(o.start_time >= 0.0)) return "start_time must be >= 0";
    if (!(o.emitter_lifetime > 0.0f) || !(o.lifetime > 0.0f)) return "emitter_lifetime and lifetime must be > 0";
    if (!(o.lifetime_randomness >= 0.0f && o.lifetime_randomness <= 1.0f)) return "lifetime_randomness outside [0, 1]";
    if (o.reserved0 != 0u) return "reserved words must be 0";
    for (uint32_t r : o.reserved)
        if (r != 0u) return "reserved words must be 0";
    SprayParams p;
    __builtin_memset(&p, 0, sizeof(p));
    for (int k = 0; k < 3; ++k) {
        const double c[3] = {o.emission_transform[k], o.emission_transform[4 + k], o.emission_transform[8 + k]};
        const double len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        if (!(len > 0.0)) return "the emission basis has a zero column";
        for (int r = 0; r < 3; ++r) p.axis[k][r] = (float)(c[r] / len);
    }
    p.amount = o.amount;
    const uint32_t np = o.num_particles ? o.num_particles : o.amount;
    p.t = (uint32_t)sqrtf((float)np);
    if (p.t < 2u) return "num_particles must be 0 or >= 4";
    p.seed = o.random_seed;
    p.emitter_lifetime = o.emitter_lifetime;
    p.lifetime = o.lifetime;
    p.randomness = o.lifetime_randomness;
    for (int k = 0; k < 3; ++k) p.particle_scale[k] = o.particle_scale[k];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) p.E[r][k] = o.emission_transform[4 * r + k];
    *P = p;
    *H = SprayHostState();
    H->time = o.start_time;
    H->cycle = std::floor(o.start_time / (double)o.emitter_lifetime);
    return nullptr;
}

inline bool spray_delta_ok(const SprayParams &P, double delta) { return std::isfinite(delta) && delta > 0.0 && delta < (double)P.emitter_lifetime; }

// the smallest i in [0, amount] with (float)i / (float)amount >= x (the quotient does not decrease with i)
inline uint32_t spray_first_at_least(uint32_t amount, float x) {
    uint32_t lo = 0, hi = amount;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((float)mid / (float)amount >= x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// advances the host's clock by delta (spray_delta_ok) and returns the step's clock; counts the step and the particles it restarts
inline SprayClock spray_advance(const SprayParams &P, SprayHostState &H, double delta) {
    const double L = (double)P.emitter_lifetime;
    const double t = H.time + delta;
    const double cycle = std::floor(t / L);
    SprayClock K;
    K.time = (float)t;
    K.utime = K.time < 4294967296.0f ? (uint32_t)K.time : 0xFFFFFFFFu;
    K.prev = H.prev;
    K.phase = (float)(std::fmod(t, L) / L);
    K.wrapped = cycle > H.cycle ? 1 : 0;
    K.base = (uint32_t)((uint64_t)std::fmod(cycle, 4294967296.0) * (uint64_t)P.amount);
    const uint32_t a = spray_first_at_least(P.amount, K.prev), b = spray_first_at_least(P.amount, K.phase);
    H.restarts += K.wrapped ? (uint64_t)(P.amount - a) + b : (uint64_t)(b > a ? b - a : 0u);
    H.time = t;
    H.cycle = cycle;
    H.prev = K.phase;
    H.steps += 1;
    return K;
}

}  // namespace ow
