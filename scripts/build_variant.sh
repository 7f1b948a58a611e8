#!/bin/bash
# developer tool: build libocean_waves with extra -D flags into godotoceanwaves_amd/csrc/build/variants/<name>.so
#   scripts/build_variant.sh map1 -DOW_P1C_MAP=1 ;  OCEAN_WAVES_LIB=.../variants/map1.so python scripts/mode_bench.py ...
# The units, their per-unit flags and the common flags are build.py's (UNITS, COMMON): the one list.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd); C=$ROOT/godotoceanwaves_amd/csrc; name=$1; shift
out=$C/build/variants; mkdir -p $out/$name
table=$(cd "$ROOT" && python -c "from godotoceanwaves_amd.build import COMMON, UNITS
print(*COMMON)
for unit, flags in UNITS.items(): print(unit, *flags)")
F=$(head -n 1 <<<"$table"); objs=(); pids=()
while read -r unit flags; do
  obj=$out/$name/${unit%.hip}.o; objs+=($obj)
  hipcc $F $flags "$@" -c $C/$unit -o $obj & pids+=($!)
done < <(tail -n +2 <<<"$table")
for p in "${pids[@]}"; do wait $p; done   # (set -e: a unit that does not compile ends the script)
hipcc --offload-arch=gfx950 -shared -o $out/$name.so "${objs[@]}"
echo $out/$name.so
