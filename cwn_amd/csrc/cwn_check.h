// cwn_check.h -- the host-side alignment predicates of the entry points' argument checks.
//
// A null pointer counts as aligned: optional arguments are checked for presence where they are required.
// File-local names, as the per-file copies were: include and call.
#pragma once
#include <stdint.h>

namespace {

// `a`: a power of two
inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool al4(const void* p) { return aligned_to(p, 4); }
inline bool al8(const void* p) { return aligned_to(p, 8); }
inline bool al16(const void* p) { return aligned_to(p, 16); }

}  // namespace
