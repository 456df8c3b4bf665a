#!/bin/bash
# Builds a differently tuned libmcpt into montecarlopathtracing_amd/csrc/variants/libmcpt_<name>.so (select it with MCPT_LIB):
#   bash tools/build_variant.sh <name> "<extra compiler flags, e.g. -DMCPT_TRACE_DIAG>"
# HIP_ONLY="..." in the environment: flags for the device compiler alone (e.g. -mllvm options); LOGIC_FLAGS="...": wavefront_logic's own
# (unset: the Makefile's LOGICFLAGS; empty: none); TRACE_FLAGS="...": those of the trace kernels' objects (TRACEFLAGS), likewise.  All
# are part of the variant's build id.  The Makefile does the work, by the product's own rules: nothing is compiled when the variant is up
# to date, everything when its flags have changed.
set -e
name=$1; shift
args=(VARIANT="$name" EXTRA="$*" HIP_ONLY="${HIP_ONLY:-}")
[ -n "${LOGIC_FLAGS+set}" ] && args+=(LOGICFLAGS="$LOGIC_FLAGS")
[ -n "${TRACE_FLAGS+set}" ] && args+=(TRACEFLAGS="$TRACE_FLAGS")
make -C "$(dirname "$0")/../montecarlopathtracing_amd/csrc" -j "${MAX_JOBS:-8}" "${args[@]}"
echo built variants/libmcpt_$name.so
