#!/bin/bash
# Builds the host code of cc_intrinsics_batch.hip with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone
# program (main.cpp) and runs it. Host code only, no GPU needed; the other objects of the library -- the Makefile's OBJS, brought
# up to date by make first -- are linked as they are.
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
csrc="$here/../../camera_calibrator_amd/csrc"
tmp="$(mktemp -d)"
trap 'rm -rf "$tmp"' EXIT
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer"
"$HIPCC" -O1 -g -std=c++17 -fPIC -Wno-unused-value -Wno-unused-result --offload-arch=gfx950 -Xarch_host "-fsanitize=address,undefined" -Xarch_host -fno-omit-frame-pointer \
  -c "$csrc/cc_intrinsics_batch.hip" -o "$tmp/cc_intrinsics_batch_san.o"
objs=$(sed -n 's/^OBJS *= *//p' "$csrc/Makefile")
make -s -C "$csrc" $objs
others=$(for o in $objs; do [ "$o" = cc_intrinsics_batch.o ] || echo "$csrc/$o"; done)
"$HIPCC" -O1 -g -std=c++17 -x c++ $SAN -c "$here/main.cpp" -o "$tmp/main.o"
"$HIPCC" --offload-arch=gfx950 $SAN "$tmp/main.o" "$tmp/cc_intrinsics_batch_san.o" $others -ldl -pthread -Wl,-rpath,/opt/rocm/lib -o "$tmp/sanitize_intr_batch"
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$tmp/sanitize_intr_batch"
