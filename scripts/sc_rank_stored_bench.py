"""Loop discovery timings (DESIGN.md 4.9a,profiles/sc_rank_stored_notes.md).

    python scripts/sc_rank_stored_bench.py [--sizes 2000 20000] [--json OUT]
For each N (a database filled by pcr_sc_add from cheap random clouds, default parameters):
    1. rankStored(0, N, 1): median wall time of 5 calls after 2 warm-ups, the copy of the result to the host included, and the time per pair;
    2. the host loop of pcr_sc_distance over the same pairs: timed on 10 000 sampled pairs (q, i < q - 40) and SCALED to the pair count;
       the sampled pairs are also compared with the ranking's row where they are its best;
    3. N x pcr_sc_query (the reference's approximation: 10 ring-key candidates of a stale snapshot), run in full on a second database
       of the same clouds;
    4. how often query's answer is worse than the exhaustive one."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cloud(rng):
    c = np.zeros((300, 4), np.float32)
    r = rng.uniform(1.0, 85.0, 300); a = rng.uniform(-np.pi, np.pi, 300)
    c[:, 0], c[:, 1], c[:, 2] = r * np.cos(a), r * np.sin(a), rng.uniform(-2.0, 10.0, 300)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--json")
    a = ap.parse_args()
    from simpleslam_amd import ScanContext
    rng = np.random.default_rng(1)
    sc, sq = ScanContext(), ScanContext()
    res = []
    for N in a.sizes:
        while len(sc) < N:
            c = _cloud(rng)
            sc.addContext(c)
            sq.addContext(c)
        excl = 40
        pairs = sum(max(0, q - excl) for q in range(N))
        for _ in range(2):
            sc.rankStored(0, N, 1)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            idx, dist, shift = sc.rankStored(0, N, 1)
            t.append((time.perf_counter() - t0) * 1e3)
        dev_ms = float(np.median(t))
        # the host loop, sampled
        L, h = sc._lib, sc._s
        d, s = C.c_double(0), C.c_int(0)
        qs = rng.integers(excl + 1, N, 10_000)
        js = (rng.random(10_000) * (qs - excl)).astype(np.int64)
        t0 = time.perf_counter()
        ok = True
        for q, i in zip(qs.tolist(), js.tolist()):
            L.pcr_sc_distance(h, q, i, C.byref(d), C.byref(s))
            ok = ok and (d.value, i) >= (dist[q, 0], idx[q, 0]) and (i != idx[q, 0] or (d.value == dist[q, 0] and s.value == shift[q, 0]))
        host_pair_us = (time.perf_counter() - t0) * 1e6 / len(qs)
        # N x query, in full
        t0 = time.perf_counter()
        worse = answered = 0
        for q in range(N):
            m, yaw, dq = sq.query(q)
            if dq is not None:
                answered += 1
                worse += dq > dist[q, 0]
        query_ms = (time.perf_counter() - t0) * 1e3
        row = dict(N=N, pairs=pairs, rank_stored_ms=round(dev_ms, 3), all_runs_ms=[round(x, 3) for x in t], ns_per_pair=round(dev_ms * 1e6 / pairs, 3),
                   host_us_per_pair_sampled=round(host_pair_us, 2), host_loop_ms_scaled=round(host_pair_us * pairs * 1e-3, 1),
                   speedup_over_host_loop=round(host_pair_us * pairs * 1e-3 / dev_ms, 1), n_query_ms=round(query_ms, 1),
                   query_answered=answered, query_worse_than_exhaustive=int(worse), sampled_pairs_consistent=bool(ok))
        print(json.dumps(row), flush=True)
        res.append(row)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
