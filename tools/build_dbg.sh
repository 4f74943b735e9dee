#!/bin/bash
# build a measurement variant of the library: tools/build_dbg.sh NAME -DFLAG [-DFLAG...]  -> calibrating_amd/lib/dbg_NAME.so
# (load it with `python bench.py --lib calibrating_amd/lib/dbg_NAME.so`).  Every source of csrc/Makefile's SRC list is
# compiled with the flags, into an object directory of its own, so the variant exports what the product exports.
# Switches that exist (sgbm_cost.hpp, sgbm_band.hpp, remap.hip):
#   values  CAMD_COST_MAX_WAVES_RGB, CAMD_COST_MAX_WAVES_GRAY, CAMD_COST_MIN_WAVES, CAMD_COST_LDS_FLOOR_RGB, CAMD_COST_TSTORE,
#           CAMD_BAND_NT, CAMD_BAND_MIN_WAVES, CAMD_BAND_ROW_MIN_WAVES, CAMD_WTA_PADQ, CAMD_ROW_PERSIST_PRIO, BAND_RING_ROWS,
#           CAMD_REMAP_*
#   probes  (wrong results; only together with -DCAMD_MEASUREMENT_BUILD) CAMD_COST_DBG_NOSTAGE, CAMD_BAND_DBG_NOSTORE,
#           CAMD_BAND_DBG_NOBARRIER
# The kernel variants measured and closed in rounds 2-6 are listed in HISTORY.md with the commit that last compiled them.
NAME=$1; shift
cd "$(dirname "$0")/../calibrating_amd/csrc" || exit 1
make -s -j4 OUT=../lib/dbg_$NAME.so OBJDIR=../lib/dbg_$NAME EXTRA_CXXFLAGS="$*" && rm -rf ../lib/dbg_$NAME && echo built dbg_$NAME.so
