#!/bin/bash
# Builds open-diffusiongs_amd/lib/libdgs_hip_base.so = the "A" of an A/B run on the GPU box (tools/attn_ab.py, gemm_ab.py, ln_ab.py and
# ab_bench.py take both libraries; *.so is git-ignored):
#   tools/ab_build.sh dit_attention.hip [rev]   the product library with ONE csrc file taken from a git revision (default HEAD)
#                                               instead of the working tree
#   tools/ab_build.sh all [rev]                 the whole library of that revision, built in a second checkout (a change that
#                                               touches shared headers or several files)
#   then, on the GPU:   python tools/attn_ab.py open-diffusiongs_amd/lib/libdgs_hip_base.so
set -eu
f=$1; rev=${2:-HEAD}
R=$(cd "$(dirname "$0")/.." && pwd)
L=$R/open-diffusiongs_amd/lib
tmp=$(mktemp -d)
if [ "$f" = all ]; then
    mkdir -p "$L"
    git -C "$R" archive "$rev" open-diffusiongs_amd/csrc open-diffusiongs_amd/dgs_amd include | tar -x -C "$tmp"
    (cd "$tmp" && PYTHONPATH=$tmp/open-diffusiongs_amd python -c "from dgs_amd import build; build.build_hip()") > /dev/null
    cp "$tmp/open-diffusiongs_amd/lib/libdgs_hip.so" "$L/libdgs_hip_base.so"
    rm -rf "$tmp"
    echo "$L/libdgs_hip_base.so  (whole library from $rev)"
    exit 0
fi
PYTHONPATH=$R/open-diffusiongs_amd python -m dgs_amd.build > /dev/null          # objects of the working tree
git -C "$R" show "$rev:open-diffusiongs_amd/csrc/$f" > "$tmp/$f"
extra=$(python - "$f" <<'PY'
import sys
sys.path.insert(0, "open-diffusiongs_amd")
from dgs_amd import build
print(" ".join(build.FLAGS.get(sys.argv[1], [])))
PY
)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I"$R/include" -I"$R/open-diffusiongs_amd/csrc" -Wno-unused-value -Wno-unused-result \
    $extra -c "$tmp/$f" -o "$tmp/base.o" 2> /dev/null
objs=$(ls "$L"/*.o | grep -v "/${f%.hip}.o$")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$L/libdgs_hip_base.so" $objs "$tmp/base.o"
rm -rf "$tmp"
echo "$L/libdgs_hip_base.so  ($f from $rev)"
