#!/bin/bash
# Build tests/host_check/host_check.cpp, repeat_check.cpp, track_obs_check.cpp, scan_obs_check.cpp, spawn_check.cpp and sensor_check.cpp, each with the library's
# pure host code (csrc/f110_host.cpp), under AddressSanitizer and UBSan, and run them.  CPU only: no offload arch, no device, nothing preloaded.
#
#   bash scripts/host_check.sh
set -euo pipefail
REPO=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=$(mktemp -d /tmp/f110_host_check_XXXXXX)
trap 'rm -rf "$OUT"' EXIT
for prog in host_check repeat_check track_obs_check scan_obs_check spawn_check sensor_check; do
    "$HIPCC" -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-option-ignored \
        "$REPO/tests/host_check/$prog.cpp" "$REPO/f110_gymnasium_ros2_jazzy_amd/csrc/f110_host.cpp" \
        -o "$OUT/$prog"
    "$OUT/$prog"
done
