"""EarlyFusion.align_sections' kernel beside align's: the milliseconds of ef_sections_kernel for max_sections = 1, 4 and 16 next to
those of ef_align_kernel on the SAME pairs and plane ('early'), under the library's event clocks (acx_profile_*: a kernel's time alone
on the device).

    python scripts/quick_bench_ef_sections.py [--reps 3] [--out FILE]

The lists: one pair of 1024 x 1024 blocks in which the second track repeats three excerpts of the first in another order (a cover that
reorders its parts); one pair of 512 x 1024; and a list of 64 pairs among 16 tracks of 200 .. 400 blocks, every second track a reordered
version of the one before it.  Per list and setting one warm-up and `reps` timed calls; min_score = 2, min_ratio = 0, pad = 0, so that the
search runs as long as the plot has anything to report.  What one section costs beyond the first is the re-sweep of the two intervals it
split -- together fewer rows than the interval had -- and its traceback on one lane; the ratio measured is written down whatever it is.
Writes profiles/ef_sections.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acoss_amd import _lib  # noqa: E402


def _opt(name, default=None):
    if name not in sys.argv:
        return default
    k = sys.argv.index(name)
    v = sys.argv[k + 1]
    del sys.argv[k:k + 2]
    return v


REPS = int(_opt("--reps", 3))
OUT = os.path.abspath(_opt("--out") or os.path.join(ROOT, "profiles", "ef_sections.json"))
DIMS = (40, 100, 96)
PLANE = 3


def track(nb, rng):
    return dict(mfccs=rng.standard_normal((nb, DIMS[0])).astype(np.float32), ssms=(2 * rng.random((nb, DIMS[1]))).astype(np.float32),
                chromas=(rng.random((nb, DIMS[2])).astype(np.float32) ** 3 + 1e-3), chroma_med=rng.random(12) ** 2)


def reordered(src, nb, parts, rng):
    """A track of nb blocks that plays `parts` ((from, to, blocks) each) of src, noise elsewhere."""
    t = track(nb, rng)
    for a, b, m in parts:
        for key in ("mfccs", "ssms", "chromas"):
            t[key][b:b + m] = src[key][a:a + m] + 0.02 * rng.standard_normal((m, src[key].shape[1])).astype(np.float32)
    return t


rng = np.random.default_rng(2929)
tracks = [track(1024, rng)]
tracks.append(reordered(tracks[0], 1024, ((40, 600, 300), (400, 100, 250), (700, 380, 180)), rng))
tracks.append(reordered(tracks[0], 512, ((500, 20, 200), (100, 260, 220)), rng))
first = len(tracks)
for k in range(8):
    nb = int(rng.integers(200, 401))
    tracks.append(track(nb, rng))
    nb2 = int(rng.integers(200, 401))
    m = min(nb, nb2) // 3
    tracks.append(reordered(tracks[-1], nb2, ((0, nb2 - m, m), (nb - m, 0, m)), rng))
many = np.array(sorted((first + 2 * k + a, first + 2 * ((k + d) % 8) + 1 - a) for k in range(8) for d in range(4) for a in (0, 1)), np.int32)
lists = {"1024 x 1024, three reordered excerpts": np.array([(1, 0)], np.int32),
         "512 x 1024, two reordered excerpts": np.array([(2, 0)], np.int32),
         "64 pairs among 16 tracks of 200..400 blocks": many}
os.makedirs(os.path.dirname(OUT), exist_ok=True)
ctx = _lib.Context(0)
ctx.ef_upload_pool(tracks)


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


rec = {"tracks": len(tracks), "reps": REPS, "plane": "early", "options": {"min_score": 2.0, "min_ratio": 0.0, "pad": 0},
       "protocol": "event clocks on (a kernel's time alone); per list and setting one warm-up, then `reps` calls, each kernel's ms per call",
       "lists": {}}
for name, pairs in lists.items():
    al_ms, al = kernel_ms("ef_align_kernel", lambda: ctx.ef_align(pairs, plane=PLANE))
    row = {"pairs": len(pairs), "ef_align_kernel_ms": al_ms, "sections": {}}
    for S_ in (1, 4, 16):
        o = _lib.section_opts("quick_bench_ef_sections", max_sections=S_)
        ms, (got, n) = kernel_ms("ef_sections_kernel", lambda: ctx.ef_align_sections(pairs, plane=PLANE, opts=o))
        hit = al["score"] >= 2.0
        assert got[hit, 0].tobytes() == al[hit].tobytes(), "section 0 is align's record"
        row["sections"][str(S_)] = {"ef_sections_kernel_ms": ms, "found_total": int(n.sum()), "found_max": int(n.max()),
                                    "found": n.tolist() if len(n) <= 4 else None,
                                    "ratio_to_align": round(float(np.median(ms) / np.median(al_ms)), 3)}
    rec["lists"][name] = row
print(json.dumps(rec), flush=True)
ctx.close()
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", OUT)
