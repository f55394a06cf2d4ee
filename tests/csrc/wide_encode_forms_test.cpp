// wide_encode_forms_test.cpp — the served rule and the form of the wide scatter encode
// (csrc/fec_forms.hpp wide_encode_served, wide_encode_form), with no GPU.  Arguments:
//   "G k r P" quadruples: prints  served=<WideEncodeRefusal as int> wide=<WideRefusal as int>
//   "--form k r P var ..." quadruples: prints
//     supported=<0|1> passes=<n> pass_rows=<n> var=<0|1> xor_only=<0|1> pol=<bits>
// The program itself checks, for every "--form" quadruple of a served shape, what does not depend on
// the numbers' values: the passes cover rows [0, r) once, in order, in pieces of at most pass_rows
// (the walk fec_launch.hpp for_wave_passes makes of them), the form is the same whatever the packet
// size, and the served rule differs from the wide recover's only by the rows cap.
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/wide_encode_forms_test.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fec_forms.hpp"

using namespace qfec;

static int fail(const char* what) {
  std::printf("FAIL %s\n", what);
  return 1;
}

int main(int argc, char** argv) {
  int i = 1;
  for (; i + 3 < argc && std::strcmp(argv[i], "--form") != 0; i += 4) {
    const uint64_t G = std::strtoull(argv[i], nullptr, 10);
    const uint32_t k = static_cast<uint32_t>(std::atoi(argv[i + 1])), r = static_cast<uint32_t>(std::atoi(argv[i + 2]));
    const uint32_t P = static_cast<uint32_t>(std::atoi(argv[i + 3]));
    const WideEncodeRefusal e = wide_encode_served(G, k, r, P);
    const WideRefusal w = wide_served(G, k, r, P);
    // the two rules differ by the rows cap and by nothing else
    if (w == WideRefusal::kRows) {
      if (e == WideEncodeRefusal::kShape) return fail("the rows cap hides a shape refusal");
    } else if ((e == WideEncodeRefusal::kServed) != (w == WideRefusal::kServed) ||
               (e == WideEncodeRefusal::kShape) != (w == WideRefusal::kShape) ||
               (e == WideEncodeRefusal::kPacket) != (w == WideRefusal::kPacket) ||
               (e == WideEncodeRefusal::kNoGroups) != (w == WideRefusal::kNoGroups) ||
               (e == WideEncodeRefusal::kGroups) != (w == WideRefusal::kGroups)) {
      return fail("the rules differ beyond the rows cap");
    }
    std::printf("served=%d wide=%d\n", static_cast<int>(e), static_cast<int>(w));
  }
  if (i < argc && std::strcmp(argv[i], "--form") == 0) {
    for (++i; i + 3 < argc; i += 4) {
      const uint32_t k = static_cast<uint32_t>(std::atoi(argv[i])), r = static_cast<uint32_t>(std::atoi(argv[i + 1]));
      const uint32_t P = static_cast<uint32_t>(std::atoi(argv[i + 2]));
      const bool var = std::atoi(argv[i + 3]) != 0;
      const WideEncodeForm f = wide_encode_form(k, r, P, var);
      const bool served = wide_encode_served(1, k, r, P) == WideEncodeRefusal::kServed;
      if (f.supported != served) return fail("supported is the served rule");
      if (f.supported) {
        if (f.pass_rows != kWidePassRows || f.POL != kWideEncodePol || f.VAR != var || f.xor_only != (r == 1))
          return fail("form fields");
        uint32_t next = 0, passes = 0;
        for (uint32_t m0 = 0; m0 < r; m0 += f.pass_rows) {  // for_wave_passes' walk
          if (m0 != next) return fail("pass order");
          next += r - m0 < f.pass_rows ? r - m0 : f.pass_rows, ++passes;
        }
        if (next != r || passes != f.passes) return fail("the passes cover [0, r) once");
        const WideEncodeForm g = wide_encode_form(k, r, 16, var), h = wide_encode_form(k, r, 1u << 20, var);
        if (g.passes != f.passes || h.passes != f.passes || g.POL != f.POL || h.POL != f.POL) return fail("the size chooses nothing");
      } else if (f.passes != 0 || f.pass_rows != 0 || f.POL != 0 || f.VAR || f.xor_only) {
        return fail("a refused form is empty");
      }
      std::printf("supported=%d passes=%u pass_rows=%u var=%d xor_only=%d pol=%d\n", f.supported ? 1 : 0, f.passes, f.pass_rows,
                  f.VAR ? 1 : 0, f.xor_only ? 1 : 0, f.POL);
    }
  }
  std::printf("ok\n");
  return 0;
}
