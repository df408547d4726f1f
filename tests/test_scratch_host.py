"""CPU: csrc/scratch.h (pthip::Scratch, the scope guard of library scratch) in a stand-alone host program.

The program supplies its own counting pthip_alloc / pthip_free (the k-th allocation can be made to fail) and
runs a function shaped like csr_transpose in csrc/sparse.hip: eight allocations in one || chain, then three
points that can return early.  With the guard no block is live afterwards and none is freed twice, wherever the
function leaves.  The same function with hand-written frees at the end only (what csr_transpose was) is run
beside it: it leaves blocks behind from the second failed allocation on, which shows that the count would see a leak.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pytensor_amd", "csrc")

N_ALLOC, N_RETURN = 8, 3

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <set>
#include "scratch.h"

static std::set<void*> live;
static int n_alloc = 0, fail_alloc = 0, bad_free = 0;

extern "C" int pthip_alloc(size_t bytes, void** dptr) {
  if (++n_alloc == fail_alloc) return 7;
  *dptr = malloc(bytes);
  live.insert(*dptr);
  return 0;
}
extern "C" int pthip_free(void* dptr) {
  if (!dptr) return 0;
  if (!live.erase(dptr)) { bad_free++; return 1; }  // unknown or freed twice
  free(dptr);
  return 0;
}

static int fail_step = 0;
static int step(int k) { return k == fail_step ? 100 + k : 0; }  // a memset / scan that can fail

static int transpose_guard() {
  pthip::Scratch mem;
  void *keys, *vals, *keys2, *vals2, *rowid, *counts, *hist, *offs;
  int r = 0;
  if ((r = mem.alloc(64, &keys)) || (r = mem.alloc(64, &vals)) || (r = mem.alloc(64, &keys2)) || (r = mem.alloc(64, &vals2)) ||
      (r = mem.alloc(64, &rowid)) || (r = mem.alloc(32, &counts)) || (r = mem.alloc(256, &hist)) || (r = mem.alloc(260, &offs)))
    return r;
  if ((r = step(1))) return r;
  if ((r = step(2))) return r;
  if ((r = step(3))) return r;
  return 0;
}

static int transpose_by_hand() {
  void *keys = nullptr, *vals = nullptr, *keys2 = nullptr, *vals2 = nullptr, *rowid = nullptr, *counts = nullptr, *hist = nullptr,
       *offs = nullptr;
  int r = 0;
  if ((r = pthip_alloc(64, &keys)) || (r = pthip_alloc(64, &vals)) || (r = pthip_alloc(64, &keys2)) || (r = pthip_alloc(64, &vals2)) ||
      (r = pthip_alloc(64, &rowid)) || (r = pthip_alloc(32, &counts)) || (r = pthip_alloc(256, &hist)) || (r = pthip_alloc(260, &offs)))
    return r;
  if ((r = step(1))) return r;
  if ((r = step(2))) return r;
  if ((r = step(3))) return r;
  for (void* p : {keys, vals, keys2, vals2, rowid, counts, hist, offs}) pthip_free(p);
  return 0;
}

static void reset(int fa, int fs) {
  for (void* p : live) free(p);
  live.clear();
  n_alloc = bad_free = 0;
  fail_alloc = fa;
  fail_step = fs;
}
// one line per case: <form> <failing allocation> <failing step> <return code> <live blocks> <bad frees>
static void run(const char* form, int (*fn)(), int fa, int fs) {
  reset(fa, fs);
  const int rc = fn();
  printf("%s %d %d %d %zu %d\n", form, fa, fs, rc, live.size(), bad_free);
}

int main() {
  for (int form = 0; form < 2; form++) {
    const char* name = form ? "hand" : "guard";
    int (*fn)() = form ? transpose_by_hand : transpose_guard;
    run(name, fn, 0, 0);
    for (int fa = 1; fa <= 8; fa++) run(name, fn, fa, 0);
    for (int fs = 1; fs <= 3; fs++) run(name, fn, 0, fs);
  }
  {  // an early release() leaves nothing for the destructor to free again
    pthip::Scratch mem;
    void *a, *b;
    reset(0, 0);
    mem.alloc(16, &a);
    mem.alloc(16, &b);
    mem.release();
    printf("release 0 0 0 %zu %d\n", live.size(), bad_free);
  }
  printf("after 0 0 0 %zu %d\n", live.size(), bad_free);
  return 0;
}
"""


def _compiler():
    for c in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if shutil.which(c):
            return c
    return None


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """{(form, failing allocation, failing step): (return code, live blocks, bad frees)} from one run of the program"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("scratch_host")
    src, exe = d / "scratch_host.cpp", d / "scratch_host"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        form, fa, fs, rc, live, bad = line.split()
        got[(form, int(fa), int(fs))] = (int(rc), int(live), int(bad))
    return got


def test_every_way_out_frees(cases):
    assert cases[("guard", 0, 0)] == (0, 0, 0)
    for fa in range(1, N_ALLOC + 1):
        assert cases[("guard", fa, 0)] == (7, 0, 0), fa
    for fs in range(1, N_RETURN + 1):
        assert cases[("guard", 0, fs)] == (100 + fs, 0, 0), fs


def test_release_then_destructor_frees_once(cases):
    assert cases[("release", 0, 0)] == (0, 0, 0)
    assert cases[("after", 0, 0)] == (0, 0, 0)


def test_the_count_sees_what_hand_written_frees_leave_behind(cases):
    assert cases[("hand", 0, 0)] == (0, 0, 0)
    assert cases[("hand", 1, 0)] == (7, 0, 0)  # (nothing obtained yet)
    for fa in range(2, N_ALLOC + 1):
        assert cases[("hand", fa, 0)] == (7, fa - 1, 0), fa
    for fs in range(1, N_RETURN + 1):
        assert cases[("hand", 0, fs)] == (100 + fs, N_ALLOC, 0), fs
