#!/bin/bash
# Builds libvstar_hip.so (gfx950 only) in-tree next to the Python package.
#   build.sh                      every object that is out of date, the gemm4w AGPR check, the link
#   build.sh --objects NAME ...   only build/NAME.o and build/f16_NAME.o, brought up to date by the same recipe; no check, no link
set -e
cd "$(dirname "$0")"
OUT=../libvstar_hip.so
export HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -Wno-unused-value -mllvm -amdgpu-mfma-vgpr-form"
ONLY=""
if [ "$1" = --objects ]; then shift; ONLY=" $* "; fi
wanted() { [ -z "$ONLY" ] || [[ "$ONLY" == *" $1 "* ]]; }
mkdir -p build
rm -f build/gemm256a.o build/f16_gemm256a.o     # (round-3 experiment, moved to tools/experiments/gemm256a)
pids=()
HDRS="common.hpp kernels.hpp gemm_epilogue.hpp gemm256_direct_epilogue.hpp mx.hpp gemm4w_loop.inc engine_base.hpp llm_cached.hpp sample.hpp sample_core.hpp beam.hpp score.hpp spec.hpp edit.hpp logprob.hpp contrast.hpp guide.hpp tails_lp.hpp op_doors.hpp row_lse.hpp row_select.hpp ../../include/vstar_hip.h ../../include/vstar_vqa.h"
stale() {  # stale <object> <source>
  [ ! -f "$1" ] && return 0
  [ "$2" -nt "$1" ] && return 0
  for h in $HDRS; do [ -f "$h" ] && [ "$h" -nt "$1" ] && return 0; done
  return 1
}
# bf16 instantiation: every kernel file + the VSM engine and its op-level doors (ops.hip) (sample.hip / beam.hip / score.hip / spec.hip / edit.hip / logprob.hip / contrast.hip / guide.hip are dtype-explicit — one launcher per storage type — and
# built once)
# gemm4w keeps its 256 accumulators in AGPRs BEHIND the compiler's back (they are clobbers of the K-loop asm statement, read back by
# v_accvgpr_read statements in the epilogue): the compiler must never use AGPRs as VGPR spill space there — it did (a2..a9, round 6)
extra() { [[ "$1" == gemm4w* ]] && echo "-mllvm -amdgpu-spill-vgpr-to-agpr=0"; }
# (gemm4w_vit8.hip is gemm4w.hip compiled again for the W8A8 quick-GELU kernels: stale with either file)
for f in gemm gemm256 gemm4w gemm4w_vit8 norm attention elementwise decode skinny quant heads preprocess engine ops comm sample beam score spec edit logprob contrast guide; do
  if wanted $f && { stale build/$f.o $f.hip || { [ $f = gemm4w_vit8 ] && [ gemm4w.hip -nt build/$f.o ]; }; }; then
    $HIPCC $FLAGS $(extra $f) -c $f.hip -o build/$f.o & pids+=($!)
  fi
done
# fp16 instantiation (-DVSTAR_LP_F16): the dtype-generic kernel files + the VQA-LLM engine and its op-level doors (vqa_ops.hip)
for f in gemm gemm256 gemm4w norm attention elementwise decode skinny vqa_engine vqa_ops; do
  [ -f $f.hip ] || continue
  if wanted $f && stale build/f16_$f.o $f.hip; then $HIPCC $FLAGS $(extra $f) -DVSTAR_LP_F16 -c $f.hip -o build/f16_$f.o & pids+=($!); fi
done
if [ -z "$ONLY" ]; then
  # the hash of the kernel sources THIS binary is built from (vstar_amd/provenance.py::kernel_source_hash, run as a script: the one
  # copy of the algorithm), compiled into the library and exported as vstar_build_source_hash(): evidence files are stamped with the
  # LOADED library's value, so a .hip edited between building and profiling / summarising shows up as a mismatch instead of a
  # matching stamp.
  SRC_HASH=$(python3 ../provenance.py)
  cat > build/src_hash.cpp.new <<EOF2
extern "C" const char* vstar_build_source_hash(void) { return "$SRC_HASH"; }
EOF2
  if ! cmp -s build/src_hash.cpp.new build/src_hash.cpp; then mv build/src_hash.cpp.new build/src_hash.cpp; else rm build/src_hash.cpp.new; fi
  if [ ! -f build/src_hash.o ] || [ build/src_hash.cpp -nt build/src_hash.o ]; then g++ -O2 -fPIC -c build/src_hash.cpp -o build/src_hash.o; fi
fi
fail=0
for p in "${pids[@]}"; do wait $p || fail=1; done
[ $fail -eq 0 ] || { echo "build failed"; exit 1; }
[ -z "$ONLY" ] || exit 0
# the AGPR proof on the three objects that are about to be linked (tools/check_gemm4w_agpr.py: disassembles, compiles nothing): a
# compiler that parks a value in an unread accumulator fails the build here, not a test somewhere else.  Exit code 2: no llvm-objdump.
agpr=$(python3 ../../tools/check_gemm4w_agpr.py build/gemm4w.o build/f16_gemm4w.o build/gemm4w_vit8.o) && rc=0 || rc=$?
case $rc in
  0) echo "gemm4w AGPR check: $(grep -c '^ok ' <<<"$agpr") kernels ok" ;;
  2) echo "$agpr: check SKIPPED" ;;
  *) echo "$agpr"; echo "build failed: gemm4w AGPR check"; exit 1 ;;
esac
$HIPCC --offload-arch=gfx950 -shared -fPIC build/*.o -o $OUT
echo "built $(realpath $OUT)"
