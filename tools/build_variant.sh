#!/bin/bash
# A library variant for same-box A/Bs: the whole library built with extra defines into its own object directory,
# build_ab/NAME/libhermeskv.so.   tools/build_variant.sh NAME "-DX=1 -DY=2"
name=$1; defs=$2; d=build_ab/$name; mkdir -p $d
make -s -C hermes_amd/csrc -j8 BUILD=../../$d/obj OUT=../../$d/libhermeskv.so EXTRA="$defs" || exit 1
rm -rf $d/obj
