"""align_sections' sweep beside align's: the milliseconds of qmax_sections_kernel for max_sections = 1, 4 and 16 next to those of
qmax_locate_kernel on the SAME pairs, under the library's event clocks (acx_profile_*: a kernel's time alone on the device).

    python scripts/quick_bench_sections.py [--reps 3] [--out FILE]

The pairs: the two plots of tests/test_gpu_qmax_path.py::test_profile_names_the_kernel (the start and the end of one work at 249
and at 505 embedded frames, one launch for both) and one pair of 2000 pooled frames each (1991 x 1991 cells: two versions of one
work that share 1500 frames).  Per list and setting one warm-up and `reps` timed calls; min_score = 2, min_ratio = 0, pad = 0, so
that the search runs as long as the plot has anything to report.  What one section costs beyond the first is the re-sweep of the
two intervals it split -- together fewer rows than the interval had --, so max_sections = S is expected to cost a small multiple
of one sweep, not S sweeps; the ratio measured is written down whatever it is.  Writes profiles/sections_<tracks>.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acoss_amd import _lib, synth  # noqa: E402


def _opt(name, default=None):
    if name not in sys.argv:
        return default
    k = sys.argv.index(name)
    v = sys.argv[k + 1]
    del sys.argv[k:k + 2]
    return v


REPS = int(_opt("--reps", 3))
OUT = _opt("--out")
M9 = 9
# (a track of T pooled frames has T - m embedded ones; the lengths are those of the test's pool: every band class's edge, 300, 2100)
tracks, start, end = synth.work_ends([M + M9 for M in (249, 505, 761, 1017, 2041, 300, 2100)], np.random.default_rng([9, 16]))
big, bstart, bend = synth.work_ends([2000], np.random.default_rng([28, 2000]))
lists = {"249 x 249 and 505 x 505": np.array([(start[249 + M9], end[249 + M9]), (start[505 + M9], end[505 + M9])], np.int32),
         "1991 x 1991 (2000 pooled frames)": np.array([(len(tracks) + bstart[2000], len(tracks) + bend[2000])], np.int32)}
frames, offsets = synth.pack(tracks + big)
N = len(offsets) - 1
OUT = os.path.abspath(OUT or os.path.join(ROOT, "profiles", "sections_%d.json" % N))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
ctx = _lib.Context(0)
ctx.upload_pool(frames, offsets)
p = _lib.serra09_params(m=M9)
assert [ctx.serra09_embed_len(int(t), p) for t in np.diff(offsets)[[start[258], start[514], len(tracks)]]] == [249, 505, 1991]


def kernel_ms(name, call):
    ctx.profile_enable(True)
    try:
        call()                                      # warm-up
        out = []
        for _ in range(REPS):
            ctx.profile_reset()
            got = call()
            prof = ctx.profile()
            assert prof[name]["launches"] == 1
            out.append(round(prof[name]["ms"], 4))
    finally:
        ctx.profile_enable(False)
    return out, got


rec = {"tracks": N, "reps": REPS, "options": {"min_score": 2.0, "min_ratio": 0.0, "pad": 0},
       "protocol": "event clocks on (a kernel's time alone); per list and setting one warm-up, then `reps` calls, each kernel's ms per call",
       "lists": {}}
for name, pairs in lists.items():
    loc_ms, al = kernel_ms("qmax_locate_kernel", lambda: ctx.serra09_align(pairs, p))
    row = {"qmax_locate_kernel_ms": loc_ms, "sections": {}}
    for S_ in (1, 4, 16):
        o = _lib.section_opts("quick_bench_sections", max_sections=S_)
        ms, (got, n) = kernel_ms("qmax_sections_kernel", lambda: ctx.serra09_align_sections(pairs, p, o))
        assert got[:, 0].tobytes() == al.tobytes(), "section 0 is align's record"
        row["sections"][str(S_)] = {"qmax_sections_kernel_ms": ms, "found": n.tolist(),
                                    "ratio_to_locate": round(float(np.median(ms) / np.median(loc_ms)), 3)}
    rec["lists"][name] = row
print(json.dumps(rec), flush=True)
ctx.close()
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", OUT)
