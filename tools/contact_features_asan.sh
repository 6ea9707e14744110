#!/bin/bash
# AddressSanitizer on the HOST side of esme_hip_contact_features, as a stand-alone program (no Python, nothing preloaded): the host halves of
# csrc/contacts.hip and csrc/api.hip are compiled with -fsanitize=address together with tools/contact_features_asan_main.cpp, which calls the
# entry with bad arguments.  Every call returns before a launch: runs WITHOUT a GPU.
set -e
cd "$(dirname "$0")/.."
OUT=${TMPDIR:-/tmp}/esme_contact_features_asan
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
$HIPCC -O1 -g -std=c++17 --offload-arch=gfx950 -Wall -Wno-unused-function -Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer \
    -I include -I esm-efficient_amd/csrc -x hip tools/contact_features_asan_main.cpp esm-efficient_amd/csrc/contacts.hip esm-efficient_amd/csrc/api.hip \
    -fsanitize=address -o "$OUT"
ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 "$OUT"
