// gather_var_forms_dump.cpp — prints which forms csrc/fec_forms.hpp decides for the
// variable-length address-table calls (fec_recover_gather_var_rs_dev, fec_encode_gather_var_rs_dev)
// at every packet size, with no GPU: per query one line for the recover and one for the encode,
//   "gather_var k=<k> r=<r> P=<P> | <launch> ; <launch> ..."  or "... | refused"
//   "encode_var k=<k> r=<r> P=<P> | <launch> ; <launch> ..."  or "... | refused"
// each launch in the field names of quicfec.launch_trace as the launchers of fec_gather_var.hip
// record it.  tests/test_gather_var_forms.py compares every line with its table.
//
//   gather_var_forms_dump             the queries: ten shapes, P = 1..2100 and 4096, 8192, 9000
//   gather_var_forms_dump --compiled  the recover_gather_var instantiations of the library, expanded
//                                     from the list the launcher's dispatch is expanded from
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/gather_var_forms_dump.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdio>
#include <cstring>
#include <vector>

#include "fec_forms.hpp"

using namespace qfec;

namespace {

void print_recover(int k, int maxe, int pol, uint32_t m0) {
  std::printf("recover_gather_var k=%d r=%d pol=%d aux=%u", k, maxe, pol, m0);
}

void recover_query(uint32_t k, uint32_t r, uint32_t P) {
  const GatherForm f = gather_var_form(k, r, P);
  std::printf("gather_var k=%u r=%u P=%u | ", k, r, P);
  if (!f.supported) {
    std::printf("refused\n");
    return;
  }
  std::printf("classify_gather_var");
  for (uint32_t m0 = 0; m0 < r; m0 += static_cast<uint32_t>(f.MAXE)) {  // the launcher's passes of MAXE rows
    std::printf(" ; ");
    print_recover(f.K, f.MAXE, f.POL, m0);
  }
  std::printf("\n");
}

void encode_query(uint32_t k, uint32_t r, uint32_t P) {
  const GatherVarEncodeForm f = gather_var_encode_form(k, r, P);
  std::printf("encode_var k=%u r=%u P=%u | ", k, r, P);
  if (!f.supported) {
    std::printf("refused\n");
    return;
  }
  for (uint32_t p = 0; p < f.passes; ++p)  // the launcher's passes of up to 8 rows
    std::printf("%sencode_gather_var k=0 r=%u first=%d pol=%d aux=%u", p ? " ; " : "", gather_var_encode_rows(r, p),
                p == 0 ? 1 : 0, kGatherVarEncodePol, p * kGatherVarEncodeRows);
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--compiled") == 0) {
#define DUMP_GATHER_VAR(K, MAXE, POL) print_recover(K, MAXE, POL, 0), std::printf("\n");
    QFEC_GATHER_VAR_FORMS(DUMP_GATHER_VAR)
    return 0;
  }
  std::vector<uint32_t> sizes;
  for (uint32_t P = 1; P <= 2100; ++P) sizes.push_back(P);
  for (uint32_t P : {4096u, 8192u, 9000u}) sizes.push_back(P);
  const uint32_t shapes[][2] = {{10, 3}, {10, 1}, {10, 2}, {4, 2}, {20, 5}, {6, 3}, {7, 4}, {12, 6}, {12, 9}, {16, 4}};
  for (const auto& kr : shapes)
    for (uint32_t P : sizes) {
      recover_query(kr[0], kr[1], P);
      encode_query(kr[0], kr[1], P);
    }
  return 0;
}
