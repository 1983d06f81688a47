#!/bin/bash
# Builds libruserf_amd variants into $AB (default abx/: git-ignored, delete it after the A/B) for A/B
# timing within one GPU session (load one with RSF_LIB_PATH=$PWD/abx/lib_NAME.so).
# REV=<rev> builds the source as of that git revision instead of the working tree.
# Each variant is a build of its own through the Makefile (objects in $AB/build_NAME/obj), with the
# extra defines on every gossip unit (SRC=gossip, the default: gossip.hip, gossip_*.hip and the
# headers they share) or on vivaldi.hip alone (SRC=vivaldi).
# Usage: build_variants.sh name "-DFLAG=.. ..." ...
set -e
cd "$(dirname "$0")/.."
ROOT=$PWD
SRCF=${SRC:-gossip}
AB=${AB:-abx}; mkdir -p $AB
while [ $# -gt 1 ]; do
  name=$1; defs=$2; shift 2
  d=$ROOT/$AB/build_$name; mkdir -p $d
  cs=$ROOT/ruserf_amd/csrc
  if [ -n "$REV" ]; then
    rm -rf $d/src && mkdir -p $d/src && git archive "$REV" ruserf_amd/csrc include | tar -x -C $d/src
    cs=$d/src/ruserf_amd/csrc
    if [ -n "$defs" ] && ! grep -q '^EXTRA' $cs/Makefile; then
      echo "$name: the Makefile of $REV takes no EXTRA defines" >&2; exit 1
    fi
  fi
  make -s -C $cs -j16 BUILD=$d/obj OUT=$ROOT/$AB/lib_$name.so EXTRA="$defs" EXTRA_UNITS="$SRCF%"
  echo built $name
done
