"""The owning holders of the batch engine (wafer_buffers.h) on a counting fake policy: a stand-alone program under the address and
undefined-behaviour sanitizers, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wafer_amd", "csrc")

HARNESS = r"""
#include "wafer_buffers.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
using namespace wafer_eng;

static int g_allocs = 0, g_frees = 0, g_fail_after = -1, g_copies = 0;
static size_t g_last_bytes = 0;
static std::set<void *> g_live;

struct FakeMem {
    static int alloc(void **p, size_t bytes)
    {
        if (g_fail_after == 0) return 2;   // (hipErrorOutOfMemory's number; any non-zero status)
        if (g_fail_after > 0) --g_fail_after;
        *p = malloc(bytes ? bytes : 1);
        g_live.insert(*p);
        ++g_allocs;
        g_last_bytes = bytes;
        return 0;
    }
    static void free(void *p)
    {
        if (!g_live.erase(p)) {
            printf("FAIL free of a block that is not live\n");
            exit(1);
        }
        ::free(p);
        ++g_frees;
    }
};
struct FakeCopy {
    using stream = int;
    static int copy(void *dst, const void *src, size_t bytes, bool, stream)
    {
        memcpy(dst, src, bytes);
        ++g_copies;
        g_last_bytes = bytes;
        return 0;
    }
};
struct Rec40 {
    int member, k;
    double x[4];
};
static_assert(sizeof(Rec40) == 40, "a record whose size is not a power of two");

#define CHECK(cond)                                         \
    do {                                                    \
        if (!(cond)) {                                      \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                       \
        }                                                   \
    } while (0)
static bool balanced() { return g_allocs == g_frees && g_live.empty(); }

int main()
{
    using Arr = Array<double, FakeMem>;
    {   // make, destruction, make twice
        Arr a;
        CHECK(a.get() == nullptr && a.size() == 0 && a.bytes() == 0);
        CHECK(a.make(7) == 0 && a.size() == 7 && a.bytes() == 56 && g_allocs == 1);
        double *first = a.get();
        first[6] = 1.0;
        CHECK(a.make(9) == 0 && g_allocs == 2 && g_frees == 1 && !g_live.count(first));   // the first block went back
        a.reset();
        CHECK(a.get() == nullptr && a.size() == 0 && g_frees == 2);
        CHECK(a.make(3) == 0);
    }
    CHECK(balanced());
    {   // a failed make leaves an empty, usable holder
        Arr a;
        CHECK(a.make(4) == 0);
        g_fail_after = 0;
        CHECK(a.make(8) == 2 && a.get() == nullptr && a.size() == 0);
        g_fail_after = -1;
        CHECK(a.make(8) == 0 && a.size() == 8);
    }
    CHECK(balanced());
    {   // moves: the moved-from holder owns nothing and frees nothing
        Arr a;
        CHECK(a.make(5) == 0);
        double *p = a.get();
        Arr b(std::move(a));
        CHECK(a.get() == nullptr && a.size() == 0 && b.get() == p && b.size() == 5);
        Arr c;
        CHECK(c.make(2) == 0);
        const int frees = g_frees;
        c = std::move(b);   // c's own block goes back
        CHECK(g_frees == frees + 1 && c.get() == p && b.get() == nullptr);
    }
    CHECK(balanced());
    {   // a vector of holders that grows (reallocation moves them), shrinks and regrows: the clear_states case
        std::vector<Array<char, FakeMem>> slots;
        for (int l = 0; l < 5; ++l) {
            Array<char, FakeMem> s;
            CHECK(s.make(100) == 0);
            slots.push_back(std::move(s));
        }
        CHECK(g_live.size() == 5);
        slots.resize(2);
        CHECK(g_live.size() == 2);
        slots.resize(0);
        CHECK(g_live.empty());
        Array<char, FakeMem> s;
        CHECK(s.make(100) == 0);
        slots.push_back(std::move(s));
        CHECK(g_live.size() == 1);
    }
    CHECK(balanced());
    {   // grow-only: nothing at or below the capacity, the new block first, a failure keeps block, contents and capacity
        GrowArray<double, FakeMem> g;
        CHECK(g.reserve(0) == 0 && g_live.empty());
        CHECK(g.reserve(10) == 0 && g.size() == 10);
        double *p = g;
        p[9] = 42.0;
        const int allocs = g_allocs;
        CHECK(g.reserve(10) == 0 && g.reserve(3) == 0 && g.reserve(0) == 0 && g_allocs == allocs && (double *)g == p);
        g_fail_after = 0;
        CHECK(g.reserve(20) == 2 && (double *)g == p && g.size() == 10 && p[9] == 42.0 && g_live.count(p));
        g_fail_after = -1;
        CHECK(g.reserve(20) == 0 && g.size() == 20 && (double *)g != nullptr && !g_live.count(p) && g_live.size() == 1);   // usable, the old block back
        ((double *)g)[19] = 1.0;
    }
    CHECK(balanced());
    {   // the pair: both or neither, counts in elements and bytes of a 40-byte record, sub-range copies
        HostDev<Rec40, FakeMem, FakeMem, FakeCopy> t;
        CHECK(t.make(7) == 0 && t.dev.size() == 7 && t.host.size() == 7 && t.dev.bytes() == 280 && t.host.bytes() == 280 && g_live.size() == 2);
        for (int i = 0; i < 7; ++i) t[i].member = i;
        memset(t.dev.get(), 0xff, t.dev.bytes());
        CHECK(t.upload(3, 0) == 0 && g_last_bytes == 120);
        CHECK(t.dev[2].member == 2 && t.dev[3].member == -1);
        CHECK(t.upload(2, 0, 4) == 0 && g_last_bytes == 80 && t.dev[3].member == -1 && t.dev[4].member == 4 && t.dev[5].member == 5 && t.dev[6].member == -1);
        t.dev[5].member = 50;
        CHECK(t.download(1, 0, 5) == 0 && g_last_bytes == 40 && t[5].member == 50 && t[4].member == 4 && t[6].member == 6);
        g_fail_after = 1;   // the device side is made, the host side fails: neither is left
        CHECK(t.make(9) == 2 && t.dev.get() == nullptr && t.host.get() == nullptr && g_live.empty());
        g_fail_after = -1;
        CHECK(t.make(9) == 0 && t.host.size() == 9);   // a retry starts over
    }
    CHECK(balanced());
    printf("OK allocs=%d frees=%d copies=%d\n", g_allocs, g_frees, g_copies);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("buffers")
    src, exe = d / "buffers.cpp", d / "buffers"
    src.write_text(HARNESS)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)


def test_holders_on_a_counting_policy(harness):
    """every alloc matched by one free (moved-from holders, a shrunk vector of holders), make twice frees the first block, a failed
    reserve keeps pointer, contents and capacity, reserve at or below the capacity allocates nothing, the pair counts a 40-byte
    record in elements and bytes alike"""
    assert harness.returncode == 0, harness.stdout[-2000:] + harness.stderr[-3000:]
    assert harness.stdout.startswith("OK "), harness.stdout
    assert harness.stderr == ""


def test_the_header_needs_no_hip():
    text = open(os.path.join(CSRC, "wafer_buffers.h")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text
