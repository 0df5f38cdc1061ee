#!/bin/bash
# Build tests/cpp/wake_protocol.cpp (the pool's wake-up protocols of spf_amd/csrc/spf_wake.hpp under forced interleavings; CPU
# only, no HIP) twice with the system g++: plain, and with ThreadSanitizer.  With "run" both are run as well.
# usage: bash tools/wake_protocol.sh [run]   ->   tools/bin/wake_protocol, tools/bin/wake_protocol_tsan
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/bin
CXX="${CXX:-g++}"
FLAGS="-std=c++17 -Wall -Wextra -pthread -g"
for v in plain tsan; do
  out=tools/bin/wake_protocol; extra="-O2"
  if [ $v = tsan ]; then out=tools/bin/wake_protocol_tsan; extra="-O1 -fno-omit-frame-pointer -fsanitize=thread"; fi
  if [ ! -x $out ] || [ tests/cpp/wake_protocol.cpp -nt $out ] || [ spf_amd/csrc/spf_wake.hpp -nt $out ] || [ tools/wake_protocol.sh -nt $out ]; then
    "$CXX" $FLAGS $extra tests/cpp/wake_protocol.cpp -o $out
  fi
done
if [ "${1:-}" = run ]; then
  tools/bin/wake_protocol
  tools/bin/wake_protocol_tsan
fi
