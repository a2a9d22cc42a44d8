"""Prefix sharing of the dense head ("Prefix sharing"), the parts that need no GPU: the planner's
choice of J and the lane indexing (dbgphmm_amd/csrc/prefix_share.h), which sparse_dyn.hip and bwd_step share, compiled
into a stand-alone program with the host address and undefined-behaviour sanitizers, against a restatement in Python."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbgphmm_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "prefix_share.h"
// "C <div>"; then per argument triple ng N cap: "J <ng> <N> <cap> <J>"; then for J = 1..6: "G <J> <lanes> <groups>
// <bytes at N = 1000>", and for every prefix of J = 1..4 digits: "P <J> <digits, first base first> <idx> <lane of
// column 0> .. <lane of column J-1>"
int main(int argc, char **argv) {
    using namespace phmm;
    printf("C %llu %d %d\n", (unsigned long long)SHARE_MEM_DIV, SHARE_MIN_J, SHARE_MAX_J);
    for (int i = 1; i + 2 < argc; i += 3) {
        const int ng = atoi(argv[i]);
        const unsigned long long N = strtoull(argv[i + 1], nullptr, 10), cap = strtoull(argv[i + 2], nullptr, 10);
        printf("J %d %llu %llu %d\n", ng, N, cap, share_choose_j(ng, N, cap));
    }
    for (int J = 1; J <= 6; J++)
        printf("G %d %u %u %llu\n", J, share_lanes(J), share_groups(J), (unsigned long long)share_table_bytes(J, 1000));
    for (int J = 1; J <= 4; J++)
        for (unsigned code = 0; code < (1u << (2 * J)); code++) {
            uint8_t dg[6];
            printf("P %d ", J);
            for (int i = 0; i < J; i++) {
                dg[i] = (uint8_t)((code >> (2 * (J - 1 - i))) & 3u);  // any enumeration of the digit strings
                printf("%d", dg[i]);
            }
            const uint32_t idx = share_prefix_index(dg, J);
            printf(" %u", idx);
            for (int j = 0; j < J; j++) printf(" %u", share_lane_of_column(idx, j));
            for (int i = 0; i < J; i++)
                if (share_digit(idx, i) != dg[i]) return 1;
            printf("\n");
        }
    return 0;
}
"""

GIB = 1 << 30
CFG3_N, CFG5_N = 131_000, 1_300_000  # node counts of the benchmark's cfg3 and cfg5 graphs (k = 40, 1 % divergence), rounded
# (ng, N, cap): cap = the share of the table budget the virtual tables may take
PLANS = [(63, CFG3_N, 15 * GIB), (1, CFG3_N, 15 * GIB), (2, CFG3_N, 15 * GIB), (4, 5800, 15 * GIB), (17, 5800, 15 * GIB),
         (625, CFG5_N, 15 * GIB), (625, CFG5_N, 1 << 50), (625, CFG5_N, 1 * GIB), (63, CFG3_N, 0),
         (80, CFG3_N, 20 * GIB), (400, 10_000, 15 * GIB)]


def groups(J):
    return -(-4 ** J // 64)


def table_bytes(J, N):
    return groups(J) * J * N * 64 * 24


def choose_j(ng, N, cap):
    """the rule of the issue: maximise ng J - J ceil(4^J / 64) over J in 2..6 among the J whose tables fit; 0 if none
    is positive"""
    best, gain = 0, 0
    for J in range(2, 7):
        g = ng * J - J * groups(J)
        if table_bytes(J, N) <= cap and g > gain:
            best, gain = J, g
    return best


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    d = tmp_path_factory.mktemp("prefix_share")
    src, exe = d / "main.cpp", d / "prefix_share_main"
    src.write_text(MAIN)
    subprocess.check_call(cmd + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                 "-I", CSRC, str(src), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    args = [str(x) for p in PLANS for x in p]
    out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True, env=env).stdout
    return [line.split() for line in out.splitlines()]


def test_planner(program_output):
    got = {(int(t[1]), int(t[2]), int(t[3])): int(t[4]) for t in program_output if t[0] == "J"}
    assert len(got) == len(PLANS)
    for p in PLANS:
        assert got[p] == choose_j(*p), p
    assert got[63, CFG3_N, 15 * GIB] == 4   # cfg3
    assert got[1, CFG3_N, 15 * GIB] == 0    # one group: 4^2 virtual lanes are a group of their own, nothing gained
    assert got[63, CFG3_N, 0] == 0
    # cfg5: the rule alone says 6 (767 GB of virtual tables); the cap bites
    assert got[625, CFG5_N, 1 << 50] == 6 and table_bytes(6, CFG5_N) > 700 * 10 ** 9
    assert got[625, CFG5_N, 15 * GIB] == 3 and table_bytes(4, CFG5_N) > 15 * GIB >= table_bytes(3, CFG5_N)
    assert got[625, CFG5_N, 1 * GIB] == 0
    assert got[80, CFG3_N, 20 * GIB] == 5   # 80 J=5: 400 - 80 = 320 > 80 J=4: 320 - 16 = 304


def test_sizes(program_output):
    c = next(t for t in program_output if t[0] == "C")
    assert (int(c[1]), int(c[2]), int(c[3])) == (16, 2, 6)
    rows = {int(t[1]): tuple(int(x) for x in t[2:]) for t in program_output if t[0] == "G"}
    assert rows == {J: (4 ** J, groups(J), table_bytes(J, 1000)) for J in range(1, 7)}
    assert [rows[J][1] for J in range(1, 7)] == [1, 1, 1, 4, 16, 64]


def test_lane_indexing(program_output):
    """idx counts the first base as the least significant digit, and idx mod 4^(j+1) is the index of the read's
    prefix of j + 1 bases -- the lane whose first j + 1 bases are the read's -- for every j < J"""
    rows = [t for t in program_output if t[0] == "P"]
    assert len(rows) == 4 + 16 + 64 + 256
    index = {}  # digit string -> idx, over all lengths
    for t in rows:
        J, digits, idx = int(t[1]), t[2], int(t[3])
        assert len(digits) == J
        assert idx == sum(int(c) * 4 ** i for i, c in enumerate(digits))
        index[digits] = idx
    for t in rows:
        J, digits = int(t[1]), t[2]
        lanes = [int(x) for x in t[4:]]
        assert len(lanes) == J
        for j in range(J):
            assert lanes[j] == int(t[3]) % 4 ** (j + 1) == index[digits[: j + 1]]
            if j <= 2:
                assert lanes[j] < 64  # virtual group 0: one 512-byte row per node and plane for the backward loads
    for J in range(1, 5):  # a bijection between the digit strings and the lanes
        assert sorted(index["".join(map(str, d))] for d in itertools.product(range(4), repeat=J)) == list(range(4 ** J))
