// scatter_forms_dump.cpp — prints which forms csrc/fec_forms.hpp decides for the scatter recover
// (fec_recover_scatter_rs_dev) at every packet size, with no GPU: per query one line without and
// one with a length table,
//   "scatter var=<0|1> k=<k> r=<r> P=<P> | <launch> ; <launch> ..."  or "... | refused"
// each launch in the field names of quicfec.launch_trace as the launchers of fec_scatter.hip record
// it.  tests/test_scatter_forms.py compares every line with its table.
//
//   scatter_forms_dump             the queries: ten shapes, P = 1..2100 and 4096, 8192, 9000
//   scatter_forms_dump --compiled  the recover_scatter instantiations of the library, expanded from
//                                  the list the launcher's dispatch is expanded from
//   scatter_forms_dump --ids       the ScatterLaunchForm numbers
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/scatter_forms_dump.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdio>
#include <cstring>
#include <vector>

#include "fec_forms.hpp"
#include "fec_knobs.hpp"

using namespace qfec;

namespace {

void print_recover(int k, int maxe, int pol, bool var, uint32_t m0) {
  std::printf("recover_scatter k=%d r=%d first=%d pol=%d aux=%u", k, maxe, var ? 1 : 0, pol, m0);
}

void query(uint32_t k, uint32_t r, uint32_t P, bool var) {
  const ScatterForm f = scatter_form(k, r, P, var);
  std::printf("scatter var=%d k=%u r=%u P=%u | ", var ? 1 : 0, k, r, P);
  if (!f.supported) {
    std::printf("refused\n");
    return;
  }
  std::printf("classify_scatter");
  for (uint32_t m0 = 0; m0 < r; m0 += static_cast<uint32_t>(f.MAXE)) {  // the launcher's passes of MAXE rows
    std::printf(" ; ");
    print_recover(f.K, f.MAXE, f.POL, f.VAR, m0);
  }
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--compiled") == 0) {
#define DUMP_SCATTER(K, MAXE, POL, VAR) print_recover(K, MAXE, POL, VAR, 0), std::printf("\n");
    QFEC_SCATTER_FORMS(DUMP_SCATTER)
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "--ids") == 0) {
    std::printf("classify_scatter %lld\n", static_cast<long long>(ScatterLaunchForm::kClassifyScatter));
    std::printf("recover_scatter %lld\n", static_cast<long long>(ScatterLaunchForm::kRecoverScatter));
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
