#!/bin/bash
# A/B of the batch solves with cardinality_check=True: build_ab/lib_parent.so (an earlier library, its Python package
# in build_ab/parent/) against build_ab/lib_new.so and this tree's package, alternating, ROUNDS rounds, host and device input; every run is its own process under a time
# limit, and the first failure ends the script.  Lines go to OUT (tools/guard_ab.py).
#   bash tools/guard_ab.sh OUT [ROUNDS]
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$1; ROUNDS=${2:-3}
for r in $(seq 1 "$ROUNDS"); do
  for lib in parent new; do
    for inp in host device; do
      pkg=$R; [ "$lib" = parent ] && pkg=$R/build_ab/parent
      MISSLAP_LIB="$R/build_ab/lib_$lib.so" timeout -k 10 600 python "$R/tools/guard_ab.py" --label "$lib" --input "$inp" \
        --pkg "$pkg" --out "$OUT"
    done
  done
done
