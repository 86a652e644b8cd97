#!/bin/bash
# Build the library's host code and tools/ppo_epoch_host_check.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (host side only:
# the device code is compiled as always and never runs) and run the program on the CPU.  It makes no launch and needs no GPU.
# usage: tools/ppo_epoch_host_check.sh [build dir, default: a fresh temporary one]
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
out="${1:-$(mktemp -d)}"
hipcc="${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}"
san="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
mkdir -p "$out"
gcc -O1 -g -fPIC $san -c "$root/dronechase_amd/csrc/te_config.c" -o "$out/te_config.o"
# the device side with the library's own flags (dronechase_amd/build.py); the sanitizers reach the host side only
"$hipcc" --offload-arch=gfx950 -O3 -std=c++17 -fno-gpu-rdc -fno-slp-vectorize -Wno-unused-function -Xarch_host -g $(printf -- '-Xarch_host %s ' $san) \
  -I"$root/include" -c "$root/dronechase_amd/csrc/te_env.hip" -o "$out/te_env.o"
"$hipcc" -x c++ -O1 -g -std=c++17 $san -I"$root/include" -c "$root/tools/ppo_epoch_host_check.cpp" -o "$out/check.o"
"$hipcc" --offload-arch=gfx950 $san "$out/check.o" "$out/te_env.o" "$out/te_config.o" -o "$out/ppo_epoch_host_check" -lm
"$out/ppo_epoch_host_check"
