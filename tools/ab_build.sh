#!/bin/bash
# Build a variant of the library for an A/B run on one box:
#   bash tools/ab_build.sh <name> "<extra hipcc flags>"      ->  starry_process_amd/libsp_hip_<name>.so
# select it at run time with SP_LIB_VARIANT=<name> (starry_process_amd/_lib.py; debug only).
# The sources and their flags are csrc/Makefile's; the extra flags follow each file's own.  The objects go to a
# directory of their own, so the default build's objects are never touched.
set -e
name=$1; shift
obj=$(mktemp -d)
trap 'rm -rf "$obj"' EXIT
make -C "$(dirname "$0")/../starry_process_amd/csrc" -j16 OBJDIR="$obj/" OUT="../libsp_hip_$name.so" EXTRA_FLAGS="$*"
echo built starry_process_amd/libsp_hip_$name.so
