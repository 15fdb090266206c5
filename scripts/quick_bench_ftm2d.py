"""Timing of the FTM2D paths (development aid): shingle prep rate, pair rate through the pair grid with and without
the host scatter, and a whole synthetic collection (streamed prep + all pairs into an N x N float32 matrix).

    python scripts/quick_bench_ftm2d.py [--n-prep 1000] [--n-grid 15000] [--n-e2e 15000]
"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from acoss_amd import _lib  # noqa: E402

NBEATS, NFRAMES = 500, 5000


class SynthTracks(object):
    """n tracks of NFRAMES chroma frames and NBEATS beats (onsets every 10 frames), made when indexed."""

    def __init__(self, n, seed=0):
        self.n, self.seed = n, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        rng = np.random.default_rng((self.seed, i))
        X = rng.random((NFRAMES, 12), dtype=np.float32)
        return dict(chroma=X, onsets=np.arange(0, NFRAMES, NFRAMES // NBEATS, dtype=np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-prep", type=int, default=1000)
    ap.add_argument("--n-grid", type=int, default=15000)
    ap.add_argument("--n-e2e", type=int, default=15000)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    res = {}
    # --- prep: tracks held in host memory, so that only the library's time is counted
    tr = SynthTracks(a.n_prep)
    tracks = [tr[i] for i in range(a.n_prep)]
    ctx.ftm2d_upload_raw_pool(tracks[:8])                    # warm-up (module load, first allocations)
    t0 = time.time()
    ctx.ftm2d_upload_raw_pool(tracks, batch=a.batch)
    dt = time.time() - t0
    res["prep_tracks_per_s"] = a.n_prep / dt
    print("prep: %d tracks of %d beats / %d frames in %.3f s: %.0f tracks/s" % (a.n_prep, NBEATS, NFRAMES, dt, a.n_prep / dt))
    del tracks
    # --- pairs: injected shingles
    n = a.n_grid
    rng = np.random.default_rng(1)
    S = rng.random((n, 900))
    S /= np.linalg.norm(S, axis=1, keepdims=True)
    ctx.ftm2d_upload_shingles(S)
    npairs = n * (n - 1) // 2
    lengths = ctx.pool_lengths(_lib.ALGO_FTM2D)
    plan = _lib.grid_plan(lengths, _lib.ALGO_FTM2D, True, world=1)
    buf = ctx.dev_alloc(4 * int(plan["floats_per_rank"][0]))
    ctx.grid_run(plan["spec"], None, 0, buf.ptr, first=0, count=4)       # warm-up
    t0 = time.time()
    ctx.grid_run(plan["spec"], None, 0, buf.ptr)
    dt = time.time() - t0
    buf.free()
    res["grid_device_pairs_per_s"] = npairs / dt
    print("pair grid, device only (acx_grid_run): %d pairs in %.3f s: %.3g pairs/s" % (npairs, dt, npairs / dt))
    D = np.zeros((n, n), np.float32)
    t0 = time.time()
    ctx.pair_grid(_lib.ALGO_FTM2D, True, None, [D], mirror=True)
    dt = time.time() - t0
    res["grid_scatter_pairs_per_s"] = npairs / dt
    print("pair grid with host scatter + mirror (acx_pair_grid): %d pairs in %.3f s: %.3g pairs/s" % (npairs, dt, npairs / dt))
    del D
    # --- a whole synthetic collection: tracks made on the fly, streamed prep, all pairs
    n = a.n_e2e
    t0 = time.time()
    ctx.ftm2d_upload_raw_pool(SynthTracks(n, seed=2), batch=a.batch)
    t1 = time.time()
    D = np.zeros((n, n), np.float32)
    ctx.pair_grid(_lib.ALGO_FTM2D, True, None, [D], mirror=True)
    t2 = time.time()
    res.update(e2e_tracks=n, e2e_prep_s=t1 - t0, e2e_pairs_s=t2 - t1, e2e_total_s=t2 - t0)
    print("end to end, %d tracks: prep %.1f s (incl. making the synthetic chroma on the host), pairs %.1f s, total %.1f s"
          % (n, t1 - t0, t2 - t1, t2 - t0))
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
