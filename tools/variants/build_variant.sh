#!/bin/bash
# Build a library variant on the host: the in-tree objects with ONE object
# recompiled under extra defines, linked to tools/variants/lib_<tag>.so
# (same header revision, so RNVP_LIB_PATH accepts it):
#   bash tools/variants/build_variant.sh TAG OBJECT "-DNAME=VALUE ..."
# OBJECT is any object of csrc/Makefile by its name in csrc/build: a source
# (conv_tiled, wgrad; a trailing .hip is accepted) or one (dtype, configuration)
# of the deep family (conv_deep_bf16_4).
set -e
TAG=$1; OBJ=$(basename ${2%.hip} .o); DEFS=$3
C=$(cd $(dirname $0)/../../dl-normalizing-flows_amd/csrc && pwd)
V=$(cd $(dirname $0) && pwd)
make -C $C -s
W=$(mktemp -d); cp -p $C/build/*.o $W/; rm $W/$OBJ.o
make -C $C -s B=$W DEFS="$DEFS" OUT=$V/lib_$TAG.so
rm -rf $W
echo built $V/lib_$TAG.so
