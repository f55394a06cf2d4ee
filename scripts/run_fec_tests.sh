#!/usr/bin/env bash
# FEC campaign: the reference's QUIC FEC-impact loop (fixed) plus the MI355X engine legs.
#
# 1. QUIC campaign -- the reference's scripts/run_fec_tests.sh:44-139: profiles mobile /
#    satellite (emulated loss 0.05 / 0.01, latency 50 / 250 ms, :23-31) x loads light (4
#    connections, 1 stream) / medium (16, 2) x FEC none / light 0.05 / moderate 0.10 /
#    heavy 0.20 (:36-41), one `quic-test --mode=test` run each (:81-93).  Two fixes: the
#    reference passes the level as `--fec=<rate>`, but --fec is a bool alias of --enable-fec
#    (main.go:46-50), so every FEC run failed flag parsing; here FEC runs pass
#    `--enable-fec --fec-rate=<rate>` and the baseline passes neither.  And the binary
#    (./bin/quic-test, :11) is not in the snapshot: the leg runs only when $QUIC_TEST_BIN (or
#    ./bin/quic-test) exists -- a Go build of the reference with this repo's cgo files
#     -- and is skipped with a note otherwise.  --dry-run prints the exact
#    commands without running anything.
# 2. Engine legs (BASELINE.json configs) through bench.py:
#      C1  k=4 r=2, 256 B, 1k groups      host CPU: the reference's xor_packets_avx2 (oracle/_ref)
#                                         timed, byte-compared with the restatement and the GPU
#      C2  k=10 r=3, 1200 B, 1M groups    encode, device-resident           } bench.py c2c3
#      C3  same, 2 erasures per group      decode, bit-exact vs the original }
#      C4  k=20 r=5, 1200 B, 1M groups per GPU, encode                         bench.py c4
#      C5  k=10 r=3, 1200 B, satellite loss p=0.01 (and mobile p=0.05),
#          encode + decode, also timed host-resident with pinned H2D/D2H       bench.py c5 --e2e
#    and the shared batcher at the reference's call pattern (scripts/batcher_sweep.sh).
#
# usage: scripts/run_fec_tests.sh [--gpus N] [--cpu-only] [--quic-only] [--dry-run]
#                                 [--duration 60s] [--out DIR]
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
GPUS=1
CPU_ONLY=0
QUIC_ONLY=0
DRY=0
DURATION=60s
OUT="$ROOT/gpurun_out/fec_campaign"
while [ $# -gt 0 ]; do
  case "$1" in
    --gpus) GPUS="$2"; shift 2 ;;
    --cpu-only) CPU_ONLY=1; shift ;;
    --quic-only) QUIC_ONLY=1; shift ;;
    --dry-run) DRY=1; shift ;;
    --duration) DURATION="$2"; shift 2 ;;
    --out) OUT="$2"; shift 2 ;;
    *) echo "unknown argument $1" >&2; exit 2 ;;
  esac
done
cd "$ROOT"
[ "$DRY" = "1" ] || mkdir -p "$OUT"

# ---------------------------------------------------------------- 1. QUIC campaign
BIN="${QUIC_TEST_BIN:-./bin/quic-test}"
declare -A LOSS=([mobile]=0.05 [satellite]=0.01)
declare -A LATENCY=([mobile]=50ms [satellite]=250ms)
declare -A FEC_RATE=([none]=0 [light]=0.05 [moderate]=0.10 [heavy]=0.20)
PORT_BASE=9600
n=0
passed=0
failed=0
quic_run() {  # profile fec_label load connections streams
  local profile=$1 fec=$2 load=$3 conns=$4 streams=$5
  local port=$((PORT_BASE + n))
  n=$((n + 1))
  local report="$OUT/quic/fec_${profile}_${fec}_${load}.json"
  local cmd=("$BIN" --mode=test --addr="127.0.0.1:$port" --cc=bbrv3 --no-tls
             --emulate-latency="${LATENCY[$profile]}" --emulate-loss="${LOSS[$profile]}")
  if [ "$fec" != "none" ]; then
    cmd+=(--enable-fec --fec-rate="${FEC_RATE[$fec]}")
  fi
  cmd+=(--connections="$conns" --streams="$streams" --duration="$DURATION" --report="$report" --report-format=json)
  if [ "$DRY" = "1" ]; then
    echo "${cmd[*]}"
    return
  fi
  mkdir -p "$OUT/quic"
  if "${cmd[@]}" > "$OUT/quic/fec_${profile}_${fec}_${load}.log" 2>&1; then
    passed=$((passed + 1))
  else
    failed=$((failed + 1))
    echo "FAILED: ${cmd[*]}" >&2
  fi
  sleep 2  # ports of the previous run (reference :98-99)
}
if [ "$DRY" = "1" ] || [ -x "$BIN" ]; then
  echo "== QUIC FEC campaign ($BIN)" >&2
  for profile in mobile satellite; do
    for load in light medium; do
      if [ "$load" = "light" ]; then conns=4; streams=1; else conns=16; streams=2; fi
      for fec in none light moderate heavy; do
        quic_run "$profile" "$fec" "$load" "$conns" "$streams"
      done
    done
  done
  [ "$DRY" = "1" ] || echo "QUIC campaign: $n runs, $passed passed, $failed failed" >&2
else
  echo "== QUIC FEC campaign skipped: $BIN not found (build the reference with INTEGRATION.md's cgo files, or set QUIC_TEST_BIN)" >&2
fi
[ "$DRY" = "1" ] && exit 0
[ "$QUIC_ONLY" = "1" ] && exit $((failed > 0))

# ---------------------------------------------------------------- 2. engine legs
echo "== build"
python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1

echo "== C1 (host CPU via the reference's AVX2 path: k=4 r=2, 256 B, 1k groups)"
# oracle/_ref's xor_packets_avx2 timed and byte-compared with the restatement (and with
# libfec_hip.so when a GPU is usable); scripts/c1_leg.py
python scripts/c1_leg.py $([ "$CPU_ONLY" = "1" ] && echo --no-gpu) | tee "$OUT/c1.json"
[ "$CPU_ONLY" = "1" ] && exit 0

run_bench() {
  local tag="$1"; shift
  echo "== $tag (gpus=$GPUS)"
  # bench.py --gpus N starts one rank per GPU itself (no WORLD_SIZE in the environment)
  timeout -k 10 900 python bench.py --gpus "$GPUS" --full "$@" > "$OUT/$tag.json" 2> "$OUT/$tag.err"
  cat "$OUT/$tag.json"
}
run_bench c2c3 --config c2c3 --steps 30 --warmup 5
run_bench c4 --config c4 --steps 30 --warmup 5 --no-cpu-baseline
run_bench c5_satellite --config c5 --steps 30 --warmup 5 --no-cpu-baseline --e2e
run_bench c5_mobile --config c5 --loss 0.05 --steps 30 --warmup 5 --no-cpu-baseline --e2e
echo "== shared batcher at the reference's call pattern"
bash scripts/batcher_sweep.sh > "$OUT/batcher.jsonl"
cat "$OUT/batcher.jsonl"
