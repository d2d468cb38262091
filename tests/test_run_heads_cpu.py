"""CPU: the indexing of run_heads.hip under the sanitizers.  A program of its own (test_morph_cpu.build_rule_program) does on the
host what the kernel's grid does, thread by thread: the loads from at_of's clamped indices, run_is_head (csrc/morph_rule.h), the
block counts, their scan and the writes in item order, over arrays of exactly n entries, so that a load or store outside them
stops the program.  Its heads are held to numpy's at the sizes of tests/test_gpu_run_heads.py.  at_of and run_is_head are the
kernel's own; block_compact (block_scan.h) is device-only code, so its count, scan and write order are modelled here, not run."""
import subprocess

import numpy as np

from test_morph_cpu import build_rule_program

SPAN, ITEMS = 2048, 8
SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 4096, 4097)

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "morph_rule.h"
using namespace vxrt;

// run_heads_kernel and block_compact, one thread after another; emit == false counts into part, emit == true writes behind it
static void grid(const uint64_t* keys, uint32_t n, uint32_t shift, bool emit, uint64_t* part, uint64_t* out, size_t room) {
    const uint32_t blocks = (n + kMorphSpan - 1) / kMorphSpan;
    for (uint32_t b = 0; b < blocks; b++) {
        uint64_t to = emit ? part[b] : 0, kept = 0;
        for (uint32_t t = 0; t < kMorphThreads; t++) {
            const uint64_t first = uint64_t(b) * kMorphSpan + t * kMorphItems;
            uint64_t before = keys[at_of(first - 1u, n)];      // wraps at entry 0
            for (uint32_t k = 0; k < kMorphItems; k++) {
                const uint64_t i = first + k, key = keys[at_of(i, n)];
                if (run_is_head(key, before, i, n, shift)) {
                    if (emit) {
                        if (to >= room) std::abort();
                        out[to++] = key >> shift;
                    }
                    kept++;
                }
                before = key;
            }
        }
        if (!emit) part[b] = kept;
    }
}

int main() {
    unsigned n, shift;
    while (std::scanf("%u %u", &n, &shift) == 2) {
        std::unique_ptr<uint64_t[]> keys(new uint64_t[n]);      // exactly n entries: the sanitizer sees every index
        for (unsigned i = 0; i < n; i++) {
            unsigned long long k;
            if (std::scanf("%llu", &k) != 1) return 2;
            keys[i] = k;
        }
        const uint32_t blocks = (n + kMorphSpan - 1) / kMorphSpan;
        std::vector<uint64_t> part(blocks + 1);
        grid(keys.get(), n, shift, false, part.data(), nullptr, 0);
        uint64_t sum = 0;
        for (uint32_t b = 0; b <= blocks; b++) {
            const uint64_t c = b < blocks ? part[b] : 0;
            part[b] = sum;
            sum += c;
        }
        std::unique_ptr<uint64_t[]> out(new uint64_t[sum]);
        grid(keys.get(), n, shift, true, part.data(), out.get(), sum);
        for (uint64_t h = 0; h < sum; h++) std::printf("%llu\n", (unsigned long long)out[h]);
        std::printf("end %llu\n", (unsigned long long)sum);
    }
    return 0;
}
"""


def cases():
    """[(keys, shift)]: all equal, all distinct, runs of a block's and of a thread's length from entry 0 and one entry early, at every
    size; and per shift keys that differ below it only, in the bit above it only, and with bit 63 set"""
    out = []
    for n in SIZES:
        i = np.arange(n, dtype=np.uint64)
        for shift in (0, 5):
            low = i % np.uint64(1 << shift)
            out.append((np.full(n, 77 << shift, np.uint64) | low, shift))
            out.append((i << np.uint64(shift) | (i & np.uint64((1 << shift) - 1)), shift))
            for length in (SPAN, ITEMS):
                for early in (0, 1):
                    out.append((((i + np.uint64(early)) // np.uint64(length)) << np.uint64(shift) | low, shift))
    n = 2 * SPAN + 1
    i = np.arange(n, dtype=np.uint64)
    for shift in (0, 5, 12):
        out.append((np.uint64(0x1234 << shift) | i % np.uint64(1 << shift), shift))
        out.append((np.where(i < SPAN + 1, 0x40 << shift, 0x41 << shift).astype(np.uint64), shift))
        out.append((np.uint64(1 << 63) | (i // np.uint64(5)) << np.uint64(shift), shift))
    return out


def test_the_kernels_indexing_under_the_sanitizers(tmp_path):
    exe = build_rule_program(tmp_path, DRIVER)
    runs = cases()
    text = "".join(f"{len(keys)} {shift}\n" + "".join(f"{k}\n" for k in keys.tolist()) for keys, shift in runs)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), (run.returncode, run.stderr[-2000:])
    lines = iter(run.stdout.split("\n"))
    for keys, shift in runs:
        assert (keys[1:] >> np.uint64(shift) >= keys[:-1] >> np.uint64(shift)).all()
        cells = keys >> np.uint64(shift)
        want = cells[np.concatenate([[0], np.flatnonzero(cells[1:] != cells[:-1]) + 1]).astype(np.int64)].tolist()
        got = []
        for line in lines:
            if line.startswith("end"):
                assert line == f"end {len(got)}"
                break
            got.append(int(line))
        assert got == want, (len(keys), shift, len(got), len(want))
    assert next(lines) == ""
