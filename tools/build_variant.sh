#!/bin/bash
# tools/build_variant.sh <name> [-DFLAG ...] : utree_amd/libexp_<name>.so = the library with kernels.hip, lanes_kernel.hip, lanes_part.hip and dev_image.c
# compiled with extra flags (the measurement builds -DUTREE_LANES_TIMERS and -DUTREE_PHASE_TIMERS, or same-box A/B of kernel variants: UTREE_AMD_SO
# selects the library for bench.py).  The other objects are the main build's (make -C utree_amd/csrc first), listed by its Makefile; the variant's go to
# build/variant_<name>/.
set -e
N=$1; shift
R=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
O=$R/build/variant_$N
mkdir -p "$O"
cd "$R/utree_amd/csrc"
HF="-O3 -fPIC --offload-arch=gfx950 -std=c++17 -Wall -Wno-unused-parameter -Wno-unused-function"
PIDS=""
/opt/rocm/bin/hipcc $HF -mllvm -amdgpu-load-store-vectorizer=0 "$@" -c kernels.hip -o "$O/kernels.o" & PIDS="$PIDS $!"
/opt/rocm/bin/hipcc $HF "$@" -c lanes_kernel.hip -o "$O/lanes_kernel.o" & PIDS="$PIDS $!"
PARTS=""
for P in $(make -s print-lanes-parts | sed 's/lanes_part_//g; s/\.o//g'); do
    IFS=_ read W I NL BS <<< "$P"
    /opt/rocm/bin/hipcc $HF "$@" -DLANES_W=$W -DLANES_I=$I -DLANES_NL=$NL -DLANES_BS=$BS -c lanes_part.hip -o "$O/lanes_part_$P.o" & PIDS="$PIDS $!"
    PARTS="$PARTS $O/lanes_part_$P.o"
done
gcc -std=gnu11 -O2 -g -fPIC -fopenmp -I/opt/rocm/include "$@" -c dev_image.c -o "$O/dev_image.o"
for p in $PIDS; do wait $p; done
OBJS=$(for o in $(make -s print-hip-objs print-host-objs); do case $o in kernels.o|lanes_kernel.o|lanes_part_*|dev_image.o) ;; *) echo $o ;; esac; done)
gcc -shared -fopenmp -o ../libexp_$N.so "$O/kernels.o" "$O/lanes_kernel.o" $PARTS "$O/dev_image.o" $OBJS -L/opt/rocm/lib -lamdhip64 -lrccl -lstdc++ -lz -lm -lpthread -Wl,-rpath,/opt/rocm/lib
echo built libexp_$N.so
