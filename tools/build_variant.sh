#!/bin/bash
# Developer tool: build a variant of libsvr_hip.so into build_ab/ with extra compiler flags, for
# tools/ab_libs.py (interleaved A/B of several builds in one process on one box).  The sources and
# flags are the Makefile's: this script only names another object directory and library.
#   tools/build_variant.sh NAME [-DSOMETHING ...]   ->  build_ab/libsvr_hip_NAME.so
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/build_ab/obj_$name
lib=$root/build_ab/libsvr_hip_$name.so
mkdir -p "$out"
make -s -j8 -C "$root/simple-vk-renderer_amd/csrc" OBJDIR="$out" LIB="$lib" EXTRA_HIPFLAGS="$*" "$lib"
rm -rf "$out"
echo "built build_ab/libsvr_hip_$name.so"
