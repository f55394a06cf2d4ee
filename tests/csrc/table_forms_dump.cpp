// table_forms_dump.cpp — prints which forms csrc/fec_forms.hpp decides for an address-table call
// at every packet size, with no GPU: one line per query,
//   "<query> k=<k> r=<r> P=<P> | <launch> ; <launch> ..."  or "... | refused"
// each launch in the field names of quicfec.launch_trace as the call's launcher records it.  The
// four tests/test_*_forms.py compare every line with their tables.
//
//   table_forms_dump <call>             the queries: ten shapes, P = 1..2100 and 4096, 8192, 9000
//   table_forms_dump <call> --compiled  the instantiations of the call's kernel, expanded from the
//                                       list the launcher's dispatch is expanded from
//   table_forms_dump <call> --rows      the call's encode at k = 1, P = 1200 and every r in 1..63:
//                                       every pass structure (gather_var, scatter_encode)
//   table_forms_dump <call> --ids       the numbers of the call's launch forms (fec_knobs.hpp)
//
// <call> and its queries:
//   gather          fec_recover_gather_rs_dev: "gather"
//   gather_var      fec_recover_gather_var_rs_dev: "gather_var", then fec_encode_gather_var_rs_dev:
//                   "encode_var"
//   scatter         fec_recover_scatter_rs_dev without and with a length table: "scatter var=<0|1>"
//                   (the trace's `first` is the length-table flag)
//   scatter_encode  fec_encode_scatter_rs_dev without and with one: "encode_scatter var=<0|1>"
//                   (`direct` is the length-table flag)
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/table_forms_dump.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdio>
#include <cstring>
#include <vector>

#include "fec_forms.hpp"
#include "fec_knobs.hpp"
#include "forms_shapes.hpp"

using namespace qfec;

namespace {

enum class Call { kGather, kGatherVar, kScatter, kScatterEncode };

void print_recover(Call c, int k, int maxe, int pol, bool var, uint32_t m0) {
  if (c == Call::kScatter)
    std::printf("recover_scatter k=%d r=%d first=%d pol=%d aux=%u", k, maxe, var ? 1 : 0, pol, m0);
  else
    std::printf("recover_gather%s k=%d r=%d pol=%d aux=%u", c == Call::kGatherVar ? "_var" : "", k, maxe, pol, m0);
}

void print_encode(Call c, uint32_t rows, bool first, bool var, uint32_t row0) {
  if (c == Call::kScatterEncode)
    std::printf("encode_scatter k=0 r=%u first=%d pol=%d direct=%d aux=%u", rows, first ? 1 : 0, kTableEncodePol,
                var ? 1 : 0, row0);
  else
    std::printf("encode_gather_var k=0 r=%u first=%d pol=%d aux=%u", rows, first ? 1 : 0, kTableEncodePol, row0);
}

// "<name> " or, for the calls with a nullable length table, "<name> var=<0|1> "
void print_query(const char* name, bool flagged, bool var, uint32_t k, uint32_t r, uint32_t P) {
  std::printf("%s ", name);
  if (flagged) std::printf("var=%d ", var ? 1 : 0);
  std::printf("k=%u r=%u P=%u | ", k, r, P);
}

void recover_query(Call c, uint32_t k, uint32_t r, uint32_t P, bool var) {
  const TableRecoverForm f = table_recover_form(k, r, P, var);
  print_query(c == Call::kGather ? "gather" : c == Call::kGatherVar ? "gather_var" : "scatter", c == Call::kScatter, var, k, r, P);
  if (!f.supported) {
    std::printf("refused\n");
    return;
  }
  std::fputs(c == Call::kGather ? "classify_gather" : c == Call::kGatherVar ? "classify_gather_var" : "classify_scatter", stdout);
  for (uint32_t m0 = 0; m0 < r; m0 += static_cast<uint32_t>(f.MAXE)) {  // the launcher's passes of MAXE rows
    std::printf(" ; ");
    print_recover(c, f.K, f.MAXE, f.POL, f.VAR, m0);
  }
  std::printf("\n");
}

void encode_query(Call c, uint32_t k, uint32_t r, uint32_t P, bool var) {
  const TableEncodeForm f = table_encode_form(k, r, P, var);
  print_query(c == Call::kGatherVar ? "encode_var" : "encode_scatter", c == Call::kScatterEncode, var, k, r, P);
  if (!f.supported) {
    std::printf("refused\n");
    return;
  }
  for (uint32_t p = 0; p < f.passes; ++p) {  // the launcher's passes of up to 8 rows
    if (p) std::printf(" ; ");
    print_encode(c, encode_pass_rows(r, p), p == 0, f.VAR, p * kEncodePassRows);
  }
  std::printf("\n");
}

// The lines of one (k, r, P); `recover` / `encode`: which of a call's two directions.
void query(Call c, uint32_t k, uint32_t r, uint32_t P, bool recover, bool encode) {
  if (c == Call::kGather && recover) recover_query(c, k, r, P, false);
  if (c == Call::kGatherVar && recover) recover_query(c, k, r, P, true);
  if (c == Call::kGatherVar && encode) encode_query(c, k, r, P, true);
  for (int var = 0; var < 2; ++var) {
    if (c == Call::kScatter && recover) recover_query(c, k, r, P, var != 0);
    if (c == Call::kScatterEncode && encode) encode_query(c, k, r, P, var != 0);
  }
}

void print_id(const char* name, long long id) { std::printf("%s %lld\n", name, id); }

}  // namespace

int main(int argc, char** argv) {
  const char* names[] = {"gather", "gather_var", "scatter", "scatter_encode"};
  int call = -1;
  for (int i = 0; i < 4 && argc > 1; ++i)
    if (std::strcmp(argv[1], names[i]) == 0) call = i;
  if (call < 0 || argc > 3) {
    std::fprintf(stderr, "usage: table_forms_dump gather|gather_var|scatter|scatter_encode [--compiled|--rows|--ids]\n");
    return 2;
  }
  const Call c = static_cast<Call>(call);
  const char* opt = argc > 2 ? argv[2] : "";
  if (std::strcmp(opt, "--compiled") == 0) {
#define DUMP_RECOVER(VAR, K, MAXE, POL) print_recover(c, K, MAXE, POL, VAR, 0), std::printf("\n");
#define DUMP_SCATTER(_, K, MAXE, POL) DUMP_RECOVER(false, K, MAXE, POL) DUMP_RECOVER(true, K, MAXE, POL)
#define DUMP_ENCODE(FIRST, VAR, R) print_encode(c, R, FIRST, VAR, 0), std::printf("\n");
    if (c == Call::kGather || c == Call::kGatherVar) {
      QFEC_TABLE_RECOVER_FORMS(DUMP_RECOVER, false)
    } else if (c == Call::kScatter) {
      QFEC_TABLE_RECOVER_FORMS(DUMP_SCATTER, ~)
    } else {
      QFEC_SCATTER_ENCODE_FORMS(DUMP_ENCODE)
    }
    return 0;
  }
  if (std::strcmp(opt, "--ids") == 0) {
    if (c == Call::kGather) {
      print_id("classify_gather", static_cast<long long>(GatherLaunchForm::kClassifyGather));
      print_id("recover_gather", static_cast<long long>(GatherLaunchForm::kRecoverGather));
    } else if (c == Call::kGatherVar) {
      print_id("classify_gather_var", static_cast<long long>(GatherVarLaunchForm::kClassifyGatherVar));
      print_id("recover_gather_var", static_cast<long long>(GatherVarLaunchForm::kRecoverGatherVar));
      print_id("encode_gather_var", static_cast<long long>(GatherVarLaunchForm::kEncodeGatherVar));
    } else if (c == Call::kScatter) {
      print_id("classify_scatter", static_cast<long long>(ScatterLaunchForm::kClassifyScatter));
      print_id("recover_scatter", static_cast<long long>(ScatterLaunchForm::kRecoverScatter));
    } else {
      print_id("encode_scatter", static_cast<long long>(ScatterEncodeLaunchForm::kEncodeScatter));
    }
    return 0;
  }
  if (std::strcmp(opt, "--rows") == 0 && (c == Call::kGatherVar || c == Call::kScatterEncode)) {
    for (uint32_t r = 1; r <= 63; ++r) query(c, 1, r, 1200, false, true);
    return 0;
  }
  if (*opt) {
    std::fprintf(stderr, "table_forms_dump %s: no option %s\n", names[call], opt);
    return 2;
  }
  std::vector<uint32_t> sizes;
  for (uint32_t P = 1; P <= 2100; ++P) sizes.push_back(P);
  for (uint32_t P : {4096u, 8192u, 9000u}) sizes.push_back(P);
  for (const auto& kr : kFormsShapes)
    for (uint32_t P : sizes) query(c, kr[0], kr[1], P, true, true);
  return 0;
}
