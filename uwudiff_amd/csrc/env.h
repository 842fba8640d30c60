// Cached environment switches of libuwu_hip.so (host only; shared by the .hip files through common.h and by dit.cpp).
#pragma once
#include <stdlib.h>

// ---- environment switches -------------------------------------------------------------------------------------
// Every UwuEnv switch turns a kernel path off or forces it, so that a GPU test (tests/test_gemm_gpu.py, test_kernels_gpu.py,
// test_fp8_gpu.py) can compare it with its reference kernel; the comment at each switch names the test.  The only other
// variable the library reads is UWU_DIT_SIDE_STREAMS (dit.cpp).  tests/test_cabi_symbols.py holds the list of names.
// Read once per switch and cached: a launch does not call getenv().  uwu_env_refresh() (api.cpp) bumps the generation so
// that the next use re-reads -- the tests flip switches inside one process.
int uwu_env_generation();
struct UwuEnv {
  const char* name;
  int gen = -1, ival = 0;
  bool set = false;
  char c0 = 0;
  explicit UwuEnv(const char* n) : name(n) {}
  const UwuEnv& get() {
    const int g = uwu_env_generation();
    if (gen != g) {
      const char* e = getenv(name);
      set = e != nullptr;
      c0 = e ? e[0] : 0;
      ival = e ? atoi(e) : 0;
      gen = g;
    }
    return *this;
  }
  bool is(char c) const { return set && c0 == c; }
};

