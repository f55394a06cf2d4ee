// scatter_encode_forms_dump.cpp — prints which forms csrc/fec_forms.hpp decides for the scatter
// encode (fec_encode_scatter_rs_dev) at every packet size, with no GPU: per query one line without
// and one with a length table,
//   "encode_scatter var=<0|1> k=<k> r=<r> P=<P> | <launch> ; <launch> ..."  or "... | refused"
// each launch in the field names of quicfec.launch_trace as the launcher of fec_scatter_encode.hip
// records it (`direct` is the length-table flag).  tests/test_scatter_encode_forms.py compares every
// line with its table.
//
//   scatter_encode_forms_dump             the queries: ten shapes, P = 1..2100 and 4096, 8192, 9000
//   scatter_encode_forms_dump --rows      k = 1, P = 1200 at every r in 1..63: every pass structure
//   scatter_encode_forms_dump --compiled  the encode_scatter instantiations of the library, expanded
//                                         from the list the launcher's dispatch is expanded from
//   scatter_encode_forms_dump --ids       the ScatterEncodeLaunchForm numbers
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/scatter_encode_forms_dump.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdio>
#include <cstring>
#include <vector>

#include "fec_forms.hpp"
#include "fec_knobs.hpp"

using namespace qfec;

namespace {

void print_encode(uint32_t rows, bool first, bool var, uint32_t row0) {
  std::printf("encode_scatter k=0 r=%u first=%d pol=%d direct=%d aux=%u", rows, first ? 1 : 0, kScatterEncodePol,
              var ? 1 : 0, row0);
}

void query(uint32_t k, uint32_t r, uint32_t P, bool var) {
  const ScatterEncodeForm f = scatter_encode_form(k, r, P, var);
  std::printf("encode_scatter var=%d k=%u r=%u P=%u | ", var ? 1 : 0, k, r, P);
  if (!f.supported) {
    std::printf("refused\n");
    return;
  }
  for (uint32_t p = 0; p < f.passes; ++p) {  // the launcher's passes
    if (p) std::printf(" ; ");
    print_encode(scatter_encode_rows(r, p), p == 0, f.VAR, p * kScatterEncodeRows);
  }
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--compiled") == 0) {
#define DUMP_ENCODE(R, FIRST, VAR) print_encode(R, FIRST, VAR, 0), std::printf("\n");
    QFEC_SCATTER_ENCODE_FORMS(DUMP_ENCODE)
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "--ids") == 0) {
    std::printf("encode_scatter %lld\n", static_cast<long long>(ScatterEncodeLaunchForm::kEncodeScatter));
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "--rows") == 0) {
    for (uint32_t r = 1; r <= 63; ++r) {
      query(1, r, 1200, false);
      query(1, r, 1200, true);
    }
    return 0;
  }
  std::vector<uint32_t> sizes;
  for (uint32_t P = 1; P <= 2100; ++P) sizes.push_back(P);
  for (uint32_t P : {4096u, 8192u, 9000u}) sizes.push_back(P);
  const uint32_t shapes[][2] = {{10, 3}, {10, 1}, {10, 2}, {4, 2}, {20, 5}, {6, 3}, {7, 4}, {12, 6}, {12, 9}, {16, 4}};
  for (const auto& kr : shapes)
    for (uint32_t P : sizes) {
      query(kr[0], kr[1], P, false);
      query(kr[0], kr[1], P, true);
    }
  return 0;
}
