#!/bin/bash
# Build libupsparts_hip.so for gfx950 (cross-compiles without a GPU).  Usage: build.sh [outdir]
# Files with listing gates (flags.sh: ups_file_gates) are also compiled to a device listing, which tools/check_listing.py must pass
# before the library is linked: a rebuild with another hipcc cannot silently bring back a form this tree has measured wrong.
set -e
cd "$(dirname "$0")"
OUT=${1:-.}
. ./flags.sh
B=${UPS_BUILD_DIR:-build}        # (object directory: an A/B build of the whole library keeps its own)
mkdir -p $B $OUT
# An object is compiled to $B/$f.o.tmp and becomes $B/$f.o only once its file's gate has passed: an interrupted or failed build leaves
# no up-to-date object that a later build would link without gating it.
build_one() {
  local f=$1 gates="$(ups_file_gates $1)"
  ups_quiet $HIPCC $UPS_FLAGS $(ups_file_flags $f) -c $f.hip -o $B/$f.o.tmp &
  if [ -n "$gates" ]; then
    ups_quiet $HIPCC $UPS_FLAGS $(ups_file_flags $f) -S --cuda-device-only $f.hip -o $B/$f.s &&
      python3 ../../tools/check_listing.py --rules "$gates" $B/$f.s || { wait; rm -f $B/$f.o.tmp; echo "listing gate failed for $f.hip"; return 1; }
  fi
  wait $! && mv $B/$f.o.tmp $B/$f.o
}
pids=()
for f in $UPS_SOURCES; do
  if [ ! -f $B/$f.o ] || [ $f.hip -nt $B/$f.o ] || [ common.h -nt $B/$f.o ] || [ env.h -nt $B/$f.o ] || [ tile.h -nt $B/$f.o ] || [ optim.h -nt $B/$f.o ] || [ segment_common.h -nt $B/$f.o ] || [ build.sh -nt $B/$f.o ] || [ flags.sh -nt $B/$f.o ] || [ ../../include/upsparts_hip.h -nt $B/$f.o ]; then
    build_one $f &
    pids+=($!)
  fi
done
ok=1
for p in "${pids[@]}"; do wait $p || ok=0; done
[ $ok = 1 ] || { echo "not linking"; exit 1; }
$HIPCC --offload-arch=gfx950 -shared -fPIC $B/*.o -o $OUT/libupsparts_hip.so
$HIPCC --version | head -1 > $OUT/libupsparts_hip.hipcc_version
echo "built $OUT/libupsparts_hip.so"
