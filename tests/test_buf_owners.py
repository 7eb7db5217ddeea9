"""The owners of GPU memory (keyhunt_amd/csrc/kh_buf.h) on the host, with stand-in allocators: a
reserve frees before it allocates, a failed reserve leaves the owner empty with capacity 0 and the
context's error set, and owners move without freeing twice.  No device call is made."""
import os
import shutil
import subprocess

import pytest

from keyhunt_amd import engine as E

SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "kh_gpu.h"
#include "kh_buf.h"
struct kh_ctx { std::string err; };
int kh::hip_fail(kh_ctx *c, const char *what, hipError_t e) {
  c->err = what;
  return e == hipErrorOutOfMemory ? KH_E_NOMEM : KH_E_HIP;
}
static int live = 0, max_live = 0, frees = 0;
static bool fail_next = false;
struct fake {
  static hipError_t alloc(void **p, size_t bytes) {
    if (fail_next) return hipErrorOutOfMemory;
    *p = malloc(bytes);
    if (++live > max_live) max_live = live;
    return hipSuccess;
  }
  static void free(void *p) { ::free(p); live--; frees++; }
  static constexpr const char *name = "fake";
};
#define CHECK(x) do { if (!(x)) { printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main() {
  kh_ctx c;
  {
    kh::gpu_buf<int, fake> b;
    CHECK(!b && b.cap() == 0 && b.get() == nullptr);
    CHECK(b.reserve(&c, 8) == 0 && b && b.cap() == 8 && live == 1);
    int *p = b.get();
    CHECK(b.reserve(&c, 4) == 0 && b.get() == p && b.cap() == 8);  // enough room: left alone
    CHECK(b.reserve(&c, 16) == 0 && b.cap() == 16);
    CHECK(max_live == 1 && frees == 1);                             // freed before allocated
    fail_next = true;
    CHECK(b.reserve(&c, 32) == KH_E_NOMEM);
    CHECK(!b && b.cap() == 0 && b.get() == nullptr && live == 0 && c.err == "fake");
    fail_next = false;
    CHECK(b.reserve(&c, 2) == 0 && b.cap() == 2);
    kh::gpu_buf<int, fake> m(std::move(b));
    CHECK(!b && b.cap() == 0 && m.cap() == 2 && live == 1);
    std::vector<kh::gpu_buf<int, fake>> v;
    v.push_back(std::move(m));
    v.emplace_back();
    CHECK(v[0].cap() == 2 && live == 1);
    v[1] = std::move(v[0]);
    CHECK(!v[0] && v[1].cap() == 2 && live == 1);
    v[1].reset();
    CHECK(live == 0 && v[1].cap() == 0);
    CHECK(v[1].reserve(&c, 3) == 0);
  }
  CHECK(live == 0);  // the destructors freed what was left
  printf("ok\n");
  return 0;
}
"""


def test_owners_free_before_allocating_and_empty_on_failure(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not shutil.which("g++") or not os.path.isdir(os.path.join(rocm, "include", "hip")):
        pytest.skip("no g++ or no HIP headers")
    src = tmp_path / "owners.cpp"
    src.write_text(SRC)
    exe = tmp_path / "owners"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(E.PKG, "csrc"), "-I", os.path.join(os.path.dirname(E.PKG), "include"),
                    "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
