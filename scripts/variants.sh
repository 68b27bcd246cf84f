#!/bin/bash
# Development: libnablaq variants (one -D set per variant, one object replaced), built in the container, timed on the GPU box.
#   scripts/variants.sh build FILE "name1:-DX=1" "name2:-DY=2 -DZ=3" ...     scripts/variants.sh run [bench args]
# The compiler flags, FILE's extra flags and the object list are nabladft_amd/build.py's; the other objects are those of the last in-tree build.
set -euo pipefail
cd "$(dirname "$0")/.."
D=nabladft_amd/_variants
if [ "${1:-}" = build ]; then
  F=$2; shift 2
  mapfile -t CFG < <(python -c 'import sys; from nabladft_amd import build as b; f = sys.argv[1] + ".hip"; assert f in b.SOURCES, f
print(" ".join(b.FLAGS)); print(" ".join(b.EXTRA.get(f, []))); print(" ".join(s[:-len(".hip")] for s in b.SOURCES))' "$F")
  [ ${#CFG[@]} -eq 3 ] || { echo "variants.sh: cannot read nabladft_amd/build.py for $F" >&2; exit 1; }
  FLAGS="${CFG[0]} ${CFG[1]} ${VAR_BASE_FLAGS:-}"; OBJS=${CFG[2]}
  mkdir -p $D; rm -f $D/*.so $D/*.o
  pids=()
  for v in "$@"; do
    n=${v%%:*}; x=${v#*:}
    /opt/rocm/bin/hipcc $FLAGS $x -c nabladft_amd/csrc/$F.hip -o $D/${F}_$n.o &
    pids+=($!)
  done
  for p in "${pids[@]}"; do wait "$p"; done   # a failed compile stops the script (set -e)
  for v in "$@"; do
    n=${v%%:*}
    L=""; for o in $OBJS; do if [ $o = $F ]; then L="$L $D/${F}_$n.o"; else L="$L nabladft_amd/csrc/_obj/$o.o"; fi; done
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $D/libnablaq_$n.so $L
  done
  ls $D/*.so
else
  shift || true
  mkdir -p gpurun_out
  for lib in nabladft_amd/libnablaq.so nabladft_amd/_variants/libnablaq_*.so; do
    echo "== $lib"
    NABLAQ_LIB=$PWD/$lib timeout -k 10 300 python bench.py --steps 4 --warmup 2 --full --no-side-legs --no-cpu-baseline "$@" 2>/dev/null | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); print({k:round(v,3) for k,v in d['kernel_ms_per_step'].items() if any(k.startswith(p) for p in '${VAR_KEYS:-msgf,gwr}'.split(','))}, round(d['ms_per_step'],3))"
  done
fi
