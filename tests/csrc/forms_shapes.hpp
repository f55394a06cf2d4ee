// forms_shapes.hpp — the (k, r) shapes the forms dump programs (forms_dump.cpp,
// table_forms_dump.cpp) query at every packet size: the five compiled shapes, then runtime-k ones
// of one pass (6+3, 7+4, 12+6, 16+4) and of two (12+9).  The tests' tables walk the same ten
// (tests/forms_support.py SHAPES, tests/test_gpu_forms.py DUMP_SHAPES).
#pragma once

#include <cstdint>

constexpr uint32_t kFormsShapes[][2] = {{10, 3}, {10, 1}, {10, 2}, {4, 2}, {20, 5}, {6, 3}, {7, 4}, {12, 6}, {12, 9}, {16, 4}};
