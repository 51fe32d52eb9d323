"""csrc/dispatch.h turns runtime flags into template arguments for every kernel launch that has variants.  The one bug that layer
can have is an ORDER swap (a ladder slot with two booleans exchanged compiles cleanly), so a stand-alone host program -- g++, no
HIP, address + undefined-behaviour sanitizers -- walks every runtime tuple and compares it with the compile-time tuple that arrives."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "dispatch.h"
#include <cstdio>
#include <initializer_list>
using namespace gdf_amd;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the compile-time tuple as bits, first flag lowest, under a marker bit for the number of flags
template <class... Bs>
static int encode(Bs...) {
  int code = 1 << sizeof...(Bs), i = 0;
  ((code |= (Bs::value ? 1 : 0) << i++), ...);
  return code;
}

int main() {
  int calls = 0, got = -1;
  auto f = [&](auto... Bs) { ++calls; got = encode(Bs...); return GDF_SUCCESS; };
  for (int m = 0; m < 2; ++m) CHECK(with_bools(f, m & 1) == GDF_SUCCESS && got == (2 | m));
  for (int m = 0; m < 4; ++m) CHECK(with_bools(f, m & 1, m & 2) == GDF_SUCCESS && got == (4 | m));
  for (int m = 0; m < 8; ++m) CHECK(with_bools(f, m & 1, m & 2, m & 4) == GDF_SUCCESS && got == (8 | m));
  for (int m = 0; m < 16; ++m) CHECK(with_bools(f, m & 1, m & 2, m & 4, m & 8) == GDF_SUCCESS && got == (16 | m));
  CHECK(calls == 2 + 4 + 8 + 16);
  // (the constants serve as template arguments inside the lambda, which is how the launch sites use them)
  auto as_template_arguments = [&](auto A, auto B) { got = std::integral_constant<int, A() * 2 + B()>::value; return GDF_CUDA_ERROR; };
  CHECK(with_bools(as_template_arguments, true, false) == GDF_CUDA_ERROR && got == 2);
  CHECK(with_bools(as_template_arguments, false, true) == GDF_CUDA_ERROR && got == 1);

  calls = 0;
  auto g = [&](auto V) { ++calls; got = std::integral_constant<int, V()>::value; return GDF_SUCCESS; };
  for (int v = 1; v <= 4; ++v) CHECK((with_int<1, 2, 3, 4>(v, g)) == GDF_SUCCESS && got == v);
  for (int v : {4, 8}) CHECK((with_int<4, 8>(v, g)) == GDF_SUCCESS && got == v);
  CHECK(calls == 6);
  for (int v : {0, 5, -1}) {                                          // off the list: the error, and the lambda is never called
    CHECK((with_int<1, 2, 3, 4>(v, g)) == GDF_INVALID_API_CALL);
    CHECK((with_int<4, 8>(v, g)) == GDF_INVALID_API_CALL);
  }
  CHECK(calls == 6);
  for (gdf_error e : {GDF_SUCCESS, GDF_CUDA_ERROR, GDF_MEMORYMANAGER_ERROR})      // the lambda's own return value, unchanged
    CHECK((with_int<1, 2, 3, 4>(2, [&](auto) { return e; })) == e);
  std::printf(failures ? "%d checks failed\n" : "dispatch ok\n", failures);
  return failures ? 1 : 0;
}
"""


def test_with_bools_and_with_int(tmp_path):
    src, exe = tmp_path / "dispatch_check.cpp", tmp_path / "dispatch_check"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "libgdf_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "dispatch ok", run.stdout + run.stderr
