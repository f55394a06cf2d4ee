// forms_dump.cpp — prints which kernel form csrc/fec_forms.hpp decides for every packet size,
// with no GPU: one line per query, "<query> | <launch> ; <launch> ..." or "<query> | refused",
// each launch in the field names of quicfec.launch_trace as the launchers of the kernel units
// (fec_encode.hip, fec_decode.hip, fec_decode_fused.hip, fec_runs.hip) record it.  tests/test_gpu_forms.py compares every line with its table.
//
//   forms_dump             decode (in place, slots, packed) and encode queries
//   forms_dump --packed    the packed decode queries only (run with QUICFEC_PACKED_RUNS set,
//                          built with -DQUICFEC_TEST_HOOKS)
//   forms_dump --compiled  the decode and recover_runs instantiations of the product library,
//                          expanded from the lists the launchers' dispatch is expanded from
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/forms_dump.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdio>
#include <cstring>
#include <vector>

#include "fec_forms.hpp"
#include "forms_shapes.hpp"

using namespace qfec;

namespace {

void print_decode(DecodeKernel kernel, int k, int maxe, int nm, int nt, int pol, bool direct, int scan, uint32_t m0) {
  switch (kernel) {
    case DecodeKernel::kBytes:
      std::printf("decode_bytes k=0 pol=%d", pol);
      break;
    case DecodeKernel::kTiled:
      std::printf("decode_tiled k=%d r=%d pol=%d", k, maxe, pol);
      break;
    case DecodeKernel::kFused:
      std::printf("decode_fused k=%d r=%d nm=%d nt=%d pol=%d direct=%d scan=%d aux=%u", k, maxe, nm, nt, pol, direct, scan, m0);
      break;
    case DecodeKernel::kWave:
      std::printf("decode_wave k=%d r=%d pol=%d aux=%u", k, maxe, pol, m0);
      break;
    case DecodeKernel::kV16:
      std::printf("decode_v16 k=%d r=%d aux=%u", k, maxe, m0);
      break;
    default:
      std::printf("nothing");
  }
}

void print_runs(int k, int r, int nm, int nt) {
  std::printf("recover_runs k=%d r=%d nm=%d nt=%d pol=%d", k, r, nm, nt, kNtLoad | kNtStore);
}

const uint64_t kSomeMasks[1] = {0};
uint8_t kSomeBytes[1] = {0};

void decode_query(const char* api, uint32_t k, uint32_t r, uint32_t P, uint32_t scan) {
  const bool packed = std::strcmp(api, "packed") == 0;
  const long runs_switch = test_knob(TestKnob::kPackedRuns, -1);
  DecodeLaunch a{};
  a.masks = kSomeMasks;
  a.groups = 1031;
  a.k = k, a.r = r, a.P = P;
  a.scan = scan;
  if (std::strcmp(api, "in_place") != 0) a.out = kSomeBytes, a.compact_out = true;
  const DecodeForm f = decode_form(a);
  std::printf("decode api=%s k=%u r=%u P=%u scan=%u runs=%ld | ", api, k, r, P, scan, runs_switch);
  if (packed) {
    const PackedForm pf = packed_form(a, f, runs_switch);
    if (pf == PackedForm::kRefused) {
      std::printf("refused\n");
      return;
    }
    if (pf == PackedForm::kRuns) {
      print_runs(static_cast<int>(k), static_cast<int>(r), static_cast<int>(layout_of(P).nm), static_cast<int>(layout_of(P).nt));
      std::printf("\n");
      return;
    }
    std::printf("rows_prefix ; ");
  }
  if (f.classify) std::printf("classify ; ");
  const uint32_t passes = f.kernel == DecodeKernel::kBytes || f.kernel == DecodeKernel::kTiled ? 1 : (r + f.MAXE - 1) / f.MAXE;
  for (uint32_t p = 0; p < passes; ++p) {
    if (p) std::printf(" ; ");
    print_decode(f.kernel, f.K, f.MAXE, f.NM, f.NT, f.POL, f.DIRECT, f.SCAN, p * f.MAXE);
  }
  std::printf("\n");
}

void encode_query(uint32_t k, uint32_t r, uint32_t P, int off) {
  EncodeLaunch a{};
  a.off_kind = static_cast<OffsetKind>(off);
  a.groups = 53;
  a.k = k, a.r = r, a.P = P;
  const EncodeForm f = encode_form(a);
  std::printf("encode k=%u r=%u P=%u off=%d | ", k, r, P, off);
  if (f.kernel == EncodeKernel::kBytes) {
    std::printf("encode_bytes k=0 off=%d\n", f.OFF);
  } else if (f.kernel == EncodeKernel::kBits) {
    std::printf("encode_bits k=%d r=%d off=0 pol=%d tile=%u aux=4\n", f.K, f.R, f.POL, f.tile);
  } else if (f.K > 0) {
    std::printf("encode_v16 k=%d r=%d off=%d first=1 pol=%d tile=%u aux=0\n", f.K, f.R, f.OFF, f.POL, f.tile);
  } else {
    for (uint32_t row0 = 0; row0 < r; row0 += kEncodePassRows)  // the launcher's passes of up to 8 rows
      std::printf("%sencode_v16 k=0 r=%u off=%d first=%d pol=%d tile=%u aux=%u", row0 ? " ; " : "",
                  encode_pass_rows(r, row0 / kEncodePassRows), f.OFF, row0 == 0, f.POL, f.tile, row0);
    std::printf("\n");
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--compiled") == 0) {
#define DUMP_DECODE(KERNEL, K, MAXE, NM, NT, POL, DIRECT, SCAN) \
  print_decode(DecodeKernel::KERNEL, K, MAXE, NM, NT, POL, DIRECT, SCAN, 0), std::printf("\n");
#define DUMP_RUNS(K, R, NM, NT) print_runs(K, R, NM, NT), std::printf("\n");
    QFEC_DECODE_FORMS(DUMP_DECODE)
    QFEC_RUNS_FORMS(DUMP_RUNS)
    return 0;
  }
  const bool packed_only = argc > 1 && std::strcmp(argv[1], "--packed") == 0;
  std::vector<uint32_t> sizes;
  for (uint32_t P = 1; P <= 2100; ++P) sizes.push_back(P);
  for (uint32_t P : {4096u, 8192u, 8193u, 9000u}) sizes.push_back(P);
  for (const auto& kr : kFormsShapes)
    for (uint32_t P : sizes) {
      for (uint32_t scan : {1u, kDecodeScanGroups}) {
        if (!packed_only) decode_query("in_place", kr[0], kr[1], P, scan), decode_query("slots", kr[0], kr[1], P, scan);
        decode_query("packed", kr[0], kr[1], P, scan);
      }
      for (int off = 0; off < 3 && !packed_only; ++off) encode_query(kr[0], kr[1], P, off);
    }
  return 0;
}
