// gather_forms_dump.cpp — prints which form csrc/fec_forms.hpp decides for an address-table
// recover (fec_recover_gather_rs_dev) at every packet size, with no GPU: one line per query,
// "gather k=<k> r=<r> P=<P> | <launch> ; <launch> ..." or "... | refused", each launch in the field
// names of quicfec.launch_trace as the launchers of fec_gather.hip record it.
// tests/test_gather_forms.py compares every line with its table.
//
//   gather_forms_dump             the queries: ten shapes, P = 1..2100 and 4096, 8192, 9000
//   gather_forms_dump --compiled  the recover_gather instantiations of the library, expanded from
//                                 the list the launcher's dispatch is expanded from
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/gather_forms_dump.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdio>
#include <cstring>
#include <vector>

#include "fec_forms.hpp"

using namespace qfec;

namespace {

void print_gather(int k, int maxe, int pol, uint32_t m0) {
  std::printf("recover_gather k=%d r=%d pol=%d aux=%u", k, maxe, pol, m0);
}

void gather_query(uint32_t k, uint32_t r, uint32_t P) {
  const GatherForm f = gather_form(k, r, P);
  std::printf("gather k=%u r=%u P=%u | ", k, r, P);
  if (!f.supported) {
    std::printf("refused\n");
    return;
  }
  std::printf("classify_gather");
  for (uint32_t m0 = 0; m0 < r; m0 += static_cast<uint32_t>(f.MAXE)) {  // the launcher's passes of MAXE rows
    std::printf(" ; ");
    print_gather(f.K, f.MAXE, f.POL, m0);
  }
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--compiled") == 0) {
#define DUMP_GATHER(K, MAXE, POL) print_gather(K, MAXE, POL, 0), std::printf("\n");
    QFEC_GATHER_FORMS(DUMP_GATHER)
    return 0;
  }
  std::vector<uint32_t> sizes;
  for (uint32_t P = 1; P <= 2100; ++P) sizes.push_back(P);
  for (uint32_t P : {4096u, 8192u, 9000u}) sizes.push_back(P);
  const uint32_t shapes[][2] = {{10, 3}, {10, 1}, {10, 2}, {4, 2}, {20, 5}, {6, 3}, {7, 4}, {12, 6}, {12, 9}, {16, 4}};
  for (const auto& kr : shapes)
    for (uint32_t P : sizes) gather_query(kr[0], kr[1], P);
  return 0;
}
