"""CPU: the set operations' interface (include/vxrt_setops.h) — plain C, declared once, exported with C linkage by both libraries,
refused without a context — the Python wrappers' signatures and argument checks, which run before any library call; the rule's model
(setops_model.py) against the identities the ops must satisfy; and the kernel's own arithmetic (csrc/setops_rule.h: the co-rank, the
two membership tests, the keep rule), compiled by g++ with the undefined-behaviour and address sanitizers into a program of its own
that walks two key lists tile by tile and thread by thread as the kernel's blocks do, against the model."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import ray_families as R
import setops_model as S
import transform_model as T
from conftest import ROOT
from test_components_cpu import bare_context, declared

FUNCTIONS = ["vxrt_combine_voxels_device"]
HEADER = "vxrt_setops.h"
NEW_SOURCES = ("setops.hip", "api_setops.hip", "setops.h", "setops_rule.h")
CSRC = os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc")


# ---- the header, the libraries, the wrappers ---------------------------------------------------------------------------------------
def test_header_declares_exactly_the_one_entry_point():
    assert declared(HEADER) == FUNCTIONS
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other.endswith(".h") and other != HEADER:
            assert not set(FUNCTIONS) & set(declared(other)), other
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "vxrt.h"' in text and "typedef enum vxrt_list_op" in text
    assert "last entry of a position wins" in text and "bit 7" in text and "path order" in text
    assert f'#include "{HEADER}"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc
    assert "api_setops.hip" in open(os.path.join(CSRC, "ctx.h")).read()
    assert len(declared("vxrt.h")) <= 40


def test_header_is_plain_c(tmp_path):
    hdr = os.path.join(ROOT, "include", HEADER)
    chk = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), hdr],
                         capture_output=True, text=True)
    assert chk.returncode == 0 and not chk.stderr.strip(), chk.stderr
    src = tmp_path / "c.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'typedef char ops_are_0_to_4[VXRT_LIST_UNION == 0 && VXRT_LIST_INTERSECT == 1 && VXRT_LIST_DIFFERENCE == 2 && VXRT_LIST_XOR == 3\n'
                   '                            && VXRT_LIST_CHANGED == 4 ? 1 : -1];\n'
                   'int main(void) {\n'
                   '    size_t n = 7;\n'
                   '    vxrt_list_op op = VXRT_LIST_XOR;\n'
                   '    int rc = vxrt_combine_voxels_device(0, 0, 0, 0, 0, 0, 0, (uint32_t)op, 0, 0, 0, &n);\n'
                   '    return rc == VXRT_E_INVALID && n == 7 ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)
    cpp = tmp_path / "c.cpp"
    cpp.write_text('#include "vxrt.hpp"\n'
                   'size_t f(vxrt::Context& c, const int16_t (*p)[3], const uint8_t (*m)[4], int16_t (*q)[3], uint8_t (*w)[4]) {\n'
                   '    return c.combine_voxels_device(p, nullptr, 1, p, nullptr, 1, VXRT_LIST_INTERSECT) + c.combine_voxels_device(p, m, 1, p, m, 1, VXRT_LIST_UNION, q, w, 2); }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cpp)], check=True)


def test_both_libraries_export_it_with_c_linkage(H):
    from gpu_voxel_raytracer_amd import _build
    for lib in (_build.LIB, H.variants_library()):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
        for f in FUNCTIONS:
            assert f in exported, (lib, f)          # unmangled => extern "C"
    assert H.lib().vxrt_abi_version() == 6


def test_a_null_context_is_invalid(H):
    L = H.lib()
    pos = np.zeros((2, 3), np.int16)
    mrgb = np.full((2, 4), 9, np.uint8)
    out_pos = np.full((4, 3), 0x5A5A, np.uint16)
    out_mrgb = np.full((4, 4), 0xA5, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n = C.c_size_t(7)
    for count in (2, 0, 1 << 32):
        k = C.c_size_t(count)
        for op in (0, 4, 5):
            assert L.vxrt_combine_voxels_device(None, p(pos), p(mrgb), k, p(pos), p(mrgb), k, C.c_uint32(op), p(out_pos), p(out_mrgb), C.c_size_t(4),
                                                C.byref(n)) == H.E_INVALID
            assert L.vxrt_combine_voxels_device(None, p(pos), None, k, p(pos), None, k, C.c_uint32(op), None, None, C.c_size_t(0), C.byref(n)) == H.E_INVALID
            assert L.vxrt_combine_voxels_device(None, None, None, k, None, None, k, C.c_uint32(op), None, None, C.c_size_t(0), None) == H.E_INVALID
    assert b"null context" in L.vxrt_last_error()
    assert n.value == 7 and (out_pos == 0x5A5A).all() and (out_mrgb == 0xA5).all() and not pos.any() and (mrgb == 9).all()


def test_the_new_sources_are_built_into_both_libraries():
    from gpu_voxel_raytracer_amd import _build
    for f in NEW_SOURCES:
        assert os.path.exists(os.path.join(CSRC, f)), f
    assert "setops.hip" in _build.SOURCES and "api_setops.hip" in _build.SOURCES      # the variants build takes SOURCES too
    assert "setops.h" in _build.HEADERS and "setops_rule.h" in _build.HEADERS and any(h.endswith(HEADER) for h in _build.HEADERS)
    rule = open(os.path.join(CSRC, "setops_rule.h")).read()
    assert "#include <hip" not in rule and '#include "' not in rule           # nothing from HIP, nothing of the project's


def test_the_wrapper_signatures_and_constants(H):
    assert list(inspect.signature(H.Context.combine_voxels).parameters) == ["self", "a_pos", "a_mrgb", "b_pos", "b_mrgb", "op", "cap"]
    assert inspect.signature(H.Context.combine_voxels).parameters["cap"].default is None
    assert list(inspect.signature(H.Context.count_common).parameters) == ["self", "a_pos", "b_pos"]
    assert list(inspect.signature(H.Context.diff_voxels).parameters) == ["self", "before_pos", "before_mrgb", "after_pos", "after_mrgb"]
    assert (H.LIST_UNION, H.LIST_INTERSECT, H.LIST_DIFFERENCE, H.LIST_XOR, H.LIST_CHANGED) == (0, 1, 2, 3, 4) == S.OPS


def test_the_wrappers_check_their_arguments_before_any_library_call(H):
    import torch
    ctx = bare_context(H)
    try:
        pos, mrgb = np.zeros((5, 3), np.int16), np.zeros((5, 4), np.uint8)
        bad_pos = (pos.astype(np.int32), pos.astype(np.uint16), pos.astype(np.float32), torch.zeros((5, 3), dtype=torch.int32), np.zeros(15, np.int16),
                   np.zeros((5, 4), np.int16), torch.zeros((5, 3), dtype=torch.int16), torch.zeros((3, 5), dtype=torch.int16).t())
        for bad in bad_pos:
            with pytest.raises(ValueError):
                ctx.combine_voxels(bad, None, pos, None, H.LIST_UNION)
            with pytest.raises(ValueError):
                ctx.combine_voxels(pos, None, bad, None, H.LIST_UNION)
            with pytest.raises(ValueError):
                ctx.count_common(bad, pos)
            with pytest.raises(ValueError):
                ctx.count_common(pos, bad)
            with pytest.raises(ValueError):
                ctx.diff_voxels(pos, mrgb, bad, mrgb)
        for bad in (mrgb.astype(np.int8), mrgb.astype(np.uint32), np.zeros((5, 3), np.uint8), np.zeros(20, np.uint8), np.zeros((4, 4), np.uint8),
                    torch.zeros((5, 4), dtype=torch.uint8), torch.zeros((4, 5), dtype=torch.uint8).t()):
            with pytest.raises(ValueError):
                ctx.combine_voxels(pos, bad, pos, mrgb, H.LIST_UNION)
            with pytest.raises(ValueError):
                ctx.combine_voxels(pos, mrgb, pos, bad, H.LIST_UNION)          # ... before anything is uploaded
            with pytest.raises(ValueError):
                ctx.diff_voxels(pos, bad, pos, mrgb)
        for bad in (pos.tolist(), None, "pos"):
            with pytest.raises(TypeError):
                ctx.combine_voxels(bad, None, pos, None, H.LIST_UNION)
            with pytest.raises(TypeError):
                ctx.combine_voxels(pos, None, bad, None, H.LIST_UNION)
            with pytest.raises(TypeError):
                ctx.count_common(pos, bad)
        with pytest.raises(TypeError):
            ctx.combine_voxels(pos, mrgb.tolist(), pos, mrgb, H.LIST_UNION)
        for bad in (-1, 5, 1.0, "0", None, True):
            with pytest.raises(ValueError):
                ctx.combine_voxels(pos, mrgb, pos, mrgb, bad)
        # rule 4
        with pytest.raises(ValueError):
            ctx.combine_voxels(pos, None, pos, mrgb, H.LIST_UNION)              # b_mrgb without a_mrgb
        with pytest.raises(ValueError):
            ctx.combine_voxels(pos, None, pos, None, H.LIST_CHANGED)            # CHANGED compares bytes
        for op in (H.LIST_UNION, H.LIST_XOR, H.LIST_CHANGED):
            with pytest.raises(ValueError):
                ctx.combine_voxels(pos, mrgb, pos, None, op)                    # these take bytes from B
        with pytest.raises(ValueError):
            ctx.diff_voxels(pos, None, pos, mrgb)
        with pytest.raises(ValueError):
            ctx.diff_voxels(pos, mrgb, pos, None)
        for bad in (-1, 1.5, "3", True):
            with pytest.raises(ValueError):
                ctx.combine_voxels(pos, mrgb, pos, mrgb, H.LIST_UNION, cap=bad)
    finally:
        ctx._h = None                                                     # __del__ / close() have nothing to destroy


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lists():
    rng = np.random.default_rng(3)
    pts = rng.integers(-12, 24, (4000, 3)).astype(np.int16)           # 4 000 random points of a cube of 36^3: duplicates are certain
    return {"cube16": R.scene_voxels("cube16"), "shell": T.shell(), "random": (pts, rng.integers(0, 256, (4000, 4)).astype(np.uint8))}


def as_dict(pos, mrgb):
    return {tuple(p): tuple(b) for p, b in zip(pos.tolist(), mrgb.tolist())}


def pairs(lists):
    names = list(lists)
    return [(x, y) for x in names for y in names if x != y]


def test_union_with_itself_is_the_list_deduplicated(lists):
    for name, (pos, mrgb) in lists.items():
        src = T.source_of(pos, mrgb)
        order = sorted(src, key=T.path_key)
        got_pos, got_mrgb = S.combine(pos, mrgb, pos, mrgb, S.UNION)
        assert got_pos.tolist() == [list(p) for p in order] and got_mrgb.tolist() == [list(src[p]) for p in order], name
        assert (got_mrgb[:, 0] < 0x80).all()
        empty = pos[:0], mrgb[:0]
        assert all(np.array_equal(x, y) for x, y in zip(S.combine(pos, mrgb, *empty, S.UNION), (got_pos, got_mrgb)))
        assert all(np.array_equal(x, y) for x, y in zip(S.combine(*empty, pos, mrgb, S.UNION), (got_pos, got_mrgb)))
        only, none = S.combine(pos, None, pos, None, S.UNION)
        assert none is None and np.array_equal(only, got_pos)
        assert len(S.combine(pos, mrgb, pos, mrgb, S.CHANGED)[0]) == 0 and len(S.combine(pos, mrgb, pos, mrgb, S.XOR)[0]) == 0
    assert len(T.source_of(*lists["random"])) < 4000                  # it has duplicates, and the last entry's bytes win


def test_intersect_and_xor_partition_the_union(lists):
    for x, y in pairs(lists):
        a, b = lists[x], lists[y]
        union, both, one = (S.combine(*a, *b, op) for op in (S.UNION, S.INTERSECT, S.XOR))
        su, sb, so = ({tuple(p) for p in r[0].tolist()} for r in (union, both, one))
        assert sb | so == su and not sb & so and len(sb) + len(so) == len(su), (x, y)
        # the bytes: INTERSECT's are A's, XOR's their own side's, UNION's B's where both have it
        da, db = T.source_of(*a), T.source_of(*b)
        assert as_dict(*both) == {p: da[p] for p in sb}
        assert as_dict(*one) == {p: (da[p] if p in da else db[p]) for p in so}
        assert as_dict(*union) == {**da, **db}
        # a mask gives INTERSECT and DIFFERENCE the same bytes
        assert all(np.array_equal(u, v) for u, v in zip(S.combine(*a, b[0], None, S.INTERSECT), both))
    assert len(S.combine(*lists["cube16"], *lists["random"], S.INTERSECT)[0]) > 100      # the lists do overlap


def test_difference_and_intersect_partition_a(lists):
    for x, y in pairs(lists):
        a, b = lists[x], lists[y]
        minus, both = S.combine(*a, *b, S.DIFFERENCE), S.combine(*a, *b, S.INTERSECT)
        assert {**as_dict(*minus), **as_dict(*both)} == T.source_of(*a) and len(minus[0]) + len(both[0]) == len(T.source_of(*a)), (x, y)


def test_replaying_changed_and_difference_on_a_gives_b(lists):
    for x, y in pairs(lists):
        a, b = lists[x], lists[y]
        scene = dict(T.source_of(*a))
        set_pos, set_mrgb = S.combine(*a, *b, S.CHANGED)
        clear_pos, _ = S.combine(a[0], None, b[0], None, S.DIFFERENCE)
        scene.update(as_dict(set_pos, set_mrgb))
        for p in clear_pos.tolist():
            del scene[tuple(p)]
        assert scene == T.source_of(*b), (x, y)
    # bit 7 of the material byte never makes a voxel changed; any other bit does
    pos = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.int16)
    before = np.array([[0x05, 1, 2, 3], [0x85, 1, 2, 3], [0x05, 1, 2, 3]], np.uint8)
    after = np.array([[0x85, 1, 2, 3], [0x05, 1, 2, 3], [0x45, 1, 2, 3]], np.uint8)
    got = S.combine(pos, before, pos, after, S.CHANGED)
    assert got[0].tolist() == [[7, 8, 9]] and got[1].tolist() == [[0x45, 1, 2, 3]]


# ---- the kernel's arithmetic as a host compiler reads it --------------------------------------------------------------------------
# The program takes cases "op ma mb" + ma lines "key word" + mb lines "key word" and walks each as setop_merge_kernel does: per block
# of kSetopSpan merged items the two co-ranks in the whole lists, the tile A[a0 - 1 .. a1) + B[b0 .. b1] copied into an array of
# exactly that size (the sanitizer sees a read past it), per thread merge_run on the tile, the word loads from safe indices, keep.
DRIVER = r"""
#include <cstdio>
#include <vector>
#include "setops_rule.h"
using namespace vxrt;
int main() {
    unsigned op, ma, mb;
    while (std::scanf("%u %u %u", &op, &ma, &mb) == 3) {
        std::vector<uint64_t> ka(ma ? ma : 2), kb(mb ? mb : 2);      // an empty list's allocation is readable at [0]
        std::vector<uint32_t> wa(ma ? ma : 4), wb(mb ? mb : 4);
        unsigned long long k;
        unsigned w;
        for (unsigned i = 0; i < ma; i++) { if (std::scanf("%llu %u", &k, &w) != 2) return 2; ka[i] = k; wa[i] = w; }
        for (unsigned i = 0; i < mb; i++) { if (std::scanf("%llu %u", &k, &w) != 2) return 2; kb[i] = k; wb[i] = w; }
        const uint32_t total = ma + mb;
        unsigned long kept_all = 0;
        for (uint32_t d0 = 0; d0 < total; d0 += kSetopSpan) {
            const uint32_t d1 = total - d0 > kSetopSpan ? d0 + kSetopSpan : total;
            const uint32_t a0 = merge_corank(ka.data(), ma, kb.data(), mb, d0), a1 = merge_corank(ka.data(), ma, kb.data(), mb, d1);
            const uint32_t b0 = d0 - a0, b1 = d1 - a1, na = a1 - a0, nb = b1 - b0;
            if (a1 < a0 || b1 < b0 || a1 > ma || b1 > mb) return 3;
            std::vector<uint64_t> tile(na + nb + 2);
            for (uint32_t e = 0; e < na + nb + 2; e++) {
                const bool in_a = e <= na;
                const uint32_t at = in_a ? a0 + e - 1u : b0 + (e - na - 1u);
                const uint64_t v = (in_a ? ka : kb)[safe_index(at, in_a ? ma : mb)];
                const bool there = in_a ? a0 + e != 0u : b0 + (e - na - 1u) < mb;
                tile[e] = there ? v : kSetopNoKey;
            }
            const uint32_t items = d1 - d0;
            for (uint32_t t = 0; t < kSetopThreads; t++) {
                const uint32_t diag = t * kSetopItems < items ? t * kSetopItems : items;
                const uint32_t count = items - diag < kSetopItems ? items - diag : kSetopItems;
                uint64_t key[kSetopItems];
                uint32_t own[kSetopItems], from_b, matched;
                const uint32_t live = merge_run(tile.data() + 1, na, tile.data() + 1 + na, nb, diag, count, key, own, &from_b, &matched);
                if (live != (count == 0 ? 0u : (1u << count) - 1u)) return 4;
                for (uint32_t i = 0; i < kSetopItems; i++) {
                    const bool fb = (from_b >> i & 1u) != 0u;
                    const uint32_t at = (fb ? b0 : a0) + own[i];
                    const uint32_t word = (fb ? wb : wa)[safe_index(at, fb ? mb : ma)];
                    const uint32_t other = wa[safe_index(a_index_before(d0 + diag + i, at), ma)];
                    if ((live >> i & 1u) != 0u && keep(op, fb, (matched >> i & 1u) != 0u, word == other)) {
                        std::printf("%llu %u\n", (unsigned long long)key[i], word);
                        kept_all++;
                    }
                }
            }
        }
        std::printf("end %lu\n", kept_all);
    }
    return 0;
}
"""


def straddle_lists(extra_in_b=False, differ=False):
    """B = 1 025 keys, A = B plus one key that sorts first (or the extra key in B): in the merge every equal pair then lies at the odd
    positions (2 k + 1, 2 k + 2), so every 8-item thread boundary has a pair across it, and one pair lies across merged items
    2 047 / 2 048, two blocks.  differ: the words of that pair differ.  -> (a_keys, a_words, b_keys, b_words)."""
    base = [10 + 3 * i for i in range(1025)]
    words = [0x80000000 | (7 * i + 1) & 0x7FFFFFFF for i in range(1025)]
    first, first_word = [1], [0x80123456]
    a_keys, a_words, b_keys, b_words = base, list(words), base, list(words)
    if extra_in_b:
        b_keys, b_words = first + base, first_word + b_words
    else:
        a_keys, a_words = first + base, first_word + a_words
    if differ:
        # the pair across merged items 2 047 / 2 048 is base[1023]
        b_words[b_keys.index(base[1023])] ^= 0x00010000
    return a_keys, a_words, b_keys, b_words


def key_cases():
    rng = np.random.default_rng(29)
    w = lambda n: [int(v) | 0x80000000 for v in rng.integers(0, 1 << 31, n)]       # noqa: E731
    asc = lambda n, top=1 << 20: sorted(int(v) for v in rng.choice(top, n, replace=False))   # noqa: E731
    cases = []
    cases += [([], [], [], []), ([5], w(1), [], []), ([], [], [5], w(1)), ([5], [0x80000001], [5], [0x80000001]), ([5], [0x80000001], [5], [0x80000002]),
              ([5], w(1), [6], w(1)), ([6], w(1), [5], w(1))]
    same = asc(3000)
    ww = w(3000)
    cases.append((same, ww, same, list(ww)))                                       # identical lists
    cases.append((same, ww, same, w(3000)))                                        # ... with other words
    cases.append(([2 * i for i in range(1500)], w(1500), [2 * i + 1 for i in range(1700)], w(1700)))      # disjoint, interleaved
    cases.append((list(range(2500)), w(2500), list(range(5000, 7100)), w(2100)))   # all of A before all of B
    cases.append((list(range(5000, 7100)), w(2100), list(range(2500)), w(2500)))   # ... and the reverse
    for total in (2047, 2048, 2049, 4097):
        for ma in (total // 2, 1, total - 1, 0):
            pool = asc(total)                                                      # both lists from one pool: they share keys
            a_keys = sorted(int(v) for v in rng.choice(pool, ma, replace=False))
            b_keys = sorted(int(v) for v in rng.choice(pool, total - ma, replace=False))
            cases.append((a_keys, w(ma), b_keys, w(total - ma)))
    for extra_in_b in (False, True):
        for differ in (False, True):
            cases.append(straddle_lists(extra_in_b, differ))
    for _ in range(200):
        ma, mb = (int(v) for v in rng.integers(0, 700, 2))
        top = int(rng.choice([800, 2000, 1 << 20]))
        a_keys, b_keys = asc(ma, max(top, ma)), asc(mb, max(top, mb))
        a_words = w(ma)
        lookup = dict(zip(a_keys, a_words))
        b_words = [lookup[k] if k in lookup and rng.random() < 0.5 else v for k, v in zip(b_keys, w(mb))]   # half the pairs have equal words
        cases.append((a_keys, a_words, b_keys, b_words))
    return cases


def test_the_straddle_lists_straddle():
    a_keys, _, b_keys, _ = straddle_lists()
    merged = sorted([(k, 0) for k in a_keys] + [(k, 1) for k in b_keys])
    at = {item: i for i, item in enumerate(merged)}
    pairs_at = [(at[(k, 0)], at[(k, 1)]) for k in b_keys]
    assert all(q == p + 1 and p % 8 in (1, 3, 5, 7) for p, q in pairs_at)
    assert sum(1 for p, q in pairs_at if p % 8 == 7) == 256 and (2047, 2048) in pairs_at      # a pair across every thread boundary, one across the block's


def run_rule_program(exe, cases):
    """cases: [(op, (a_keys, a_words, b_keys, b_words))] through the program (test_morph_cpu.build_rule_program of DRIVER) ->
    [[(key, word)]] per case, each held to the count the program prints behind it."""
    text = "".join(f"{op} {len(c[0])} {len(c[2])}\n" + "".join(f"{k} {v}\n" for k, v in zip(c[0], c[1])) + "".join(f"{k} {v}\n" for k, v in zip(c[2], c[3]))
                   for op, c in cases)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), run.stderr[-2000:]
    lines = iter(run.stdout.split("\n"))
    results = []
    for n, (op, c) in enumerate(cases):
        got = []
        for line in lines:
            if line.startswith("end"):
                assert line == f"end {len(got)}", (n, S.NAMES[op], line, len(got))
                break
            got.append(tuple(int(v) for v in line.split()))
        results.append(got)
    assert next(lines) == ""
    return results


def test_the_kernels_arithmetic_under_the_sanitizers(tmp_path):
    from test_morph_cpu import build_rule_program
    exe = build_rule_program(tmp_path, DRIVER)
    cases = [(op, c) for c in key_cases() for op in S.OPS]
    kept_any = {op: 0 for op in S.OPS}
    for n, ((op, c), got) in enumerate(zip(cases, run_rule_program(exe, cases))):
        want = S.combine_keys(*c, op)
        assert len(got) == len(want), (n, S.NAMES[op], len(got), len(want))
        assert got == want, (n, S.NAMES[op], len(c[0]), len(c[2]))
        kept_any[op] += len(want)
    assert all(kept_any.values())
