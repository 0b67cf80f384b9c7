#!/bin/sh
# Cache-policy sweep of the stream probe (tools/probes/probe_stream.hip, mode "policy"): store policy x load policy on the
# fused 2-D kernels' fat access shapes, and the 30 MB dependent-boundary pair.  Builds the probe when it is missing
# (hipcc cross-compiles without a device), runs it once and writes one JSON line per variant and direction.
#   tools/probe_cache_policy.sh [ROUNDS per direction, default 15] [OUTPUT, default profiles/cache_policy_probe.jsonl]
set -eu
root=$(cd "$(dirname "$0")/.." && pwd)
rounds=${1:-15}
out=${2:-$root/profiles/cache_policy_probe.jsonl}
probe=$root/tools/probes/probe_stream
if [ ! -x "$probe" ]; then
    "${HIPCC:-/opt/rocm/bin/hipcc}" -O3 -std=c++17 --offload-arch=gfx950 -o "$probe" "$probe.hip"
fi
timeout -k 10 300 "$probe" "$rounds" policy > "$out"
echo "wrote $(wc -l < "$out") lines to $out"
