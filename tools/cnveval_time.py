#!/usr/bin/env python3
"""Time gd_cnveval at the size of a 1000-Genomes evaluation ("Measured").

    python tools/cnveval_time.py [--samples 2504] [--truths 40000] [--calls 30] [--limit 300] [--out FILE]

A seeded set: truths on 22 chromosomes of 10^8 bases, lengths log-uniform from 10^3 to 10^6, copy numbers 0 .. 4, each
naming k samples with P(k > x) = 1 / x (long-tailed: most name one or two, a few name hundreds); --calls calls a sample,
half of them a truth that names the sample moved by up to 10 % of its length, half anywhere.  gd_cnveval runs once cold
and five times warm, all under one time limit (SIGALRM ends the process); gd_cnveval_timing's split of every run, the
pair count (samples with calls x truths) and the pairs per second of the kernels are printed as one JSON line.  Nothing
is checked against the Python restatement at this size (hours); the totals of all runs must agree."""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from goleft_amd import _lib                                             # noqa: E402


def make(S, T, calls, seed=2504):
    rng = np.random.default_rng(seed)
    t_chrom = rng.integers(0, 22, T).astype(np.int32)
    t_len = np.exp(rng.uniform(np.log(1e3), np.log(1e6), T)).astype(np.int64)
    t_start = rng.integers(0, 10 ** 8, T)
    t_end = t_start + t_len
    t_cn = rng.integers(0, 5, T).astype(np.int32)
    k = np.clip((rng.pareto(1.0, T) + 1).astype(np.int64), 1, S)
    t_off = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    t_samples = np.concatenate([rng.choice(S, size=n, replace=False) for n in k]).astype(np.int32)
    e_truth = np.repeat(np.arange(T), k)
    # per sample: up to calls / 2 of the truths that name it, moved; the rest anywhere
    order = rng.permutation(len(e_truth))
    order = order[np.argsort(t_samples[order], kind="stable")]
    s_sorted = t_samples[order]
    rank_in_sample = np.arange(len(order)) - np.searchsorted(s_sorted, s_sorted, side="left")
    take = order[rank_in_sample < calls // 2]
    near_s, near_t = t_samples[take], e_truth[take]
    jit = lambda n, scale: (rng.uniform(-0.1, 0.1, n) * scale).astype(np.int64)
    ns = np.maximum(0, t_start[near_t] + jit(len(take), t_len[near_t]))
    ne = np.maximum(ns, t_end[near_t] + jit(len(take), t_len[near_t]))
    n_far = S * calls - len(take)
    have = np.bincount(near_s, minlength=S)
    far_s = np.repeat(np.arange(S), calls - have)
    fl = np.exp(rng.uniform(np.log(1e3), np.log(1e6), n_far)).astype(np.int64)
    fs = rng.integers(0, 10 ** 8, n_far)
    c_sample = np.concatenate([near_s, far_s])
    c_chrom = np.concatenate([t_chrom[near_t], rng.integers(0, 22, n_far)]).astype(np.int32)
    c_start = np.concatenate([ns, fs])
    c_end = np.concatenate([ne, fs + fl])
    c_cn = np.concatenate([t_cn[near_t], rng.integers(0, 5, n_far)]).astype(np.int32)
    o = np.lexsort((c_start, c_chrom, c_sample))
    cnv_off = np.concatenate([[0], np.cumsum(np.bincount(c_sample, minlength=S))]).astype(np.int64)
    i32 = lambda x: np.ascontiguousarray(x, np.int32)
    return [cnv_off, i32(c_chrom[o]), i32(c_start[o]), i32(c_end[o]), i32(c_cn[o]), i32(t_chrom), i32(t_start), i32(t_end), i32(t_cn),
            t_off, i32(t_samples)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--truths", type=int, default=40000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--limit", type=int, default=300, help="seconds for everything")
    ap.add_argument("--out")
    a = ap.parse_args()
    signal.alarm(a.limit)
    S, T = a.samples, a.truths
    t0 = time.perf_counter()
    arrays = make(S, T, a.calls)
    res = dict(samples=S, truths=T, calls=int(arrays[0][-1]), entries=int(arrays[9][-1]), make_s=round(time.perf_counter() - t0, 3))
    active = int((np.diff(arrays[0]) > 0).sum())
    res["pairs"] = active * T
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.gd_create(0, C.byref(h)) == 0
    runs, totals = [], []
    for _ in range(6):
        stats = np.zeros((S, 3, 4), np.int64)
        t0 = time.perf_counter()
        rc = lib.gd_cnveval(h, S, *[x.ctypes.data for x in arrays[:5]], T, *[x.ctypes.data for x in arrays[5:]], 0.4, stats.ctypes.data)
        wall = time.perf_counter() - t0
        assert rc == 0, lib.gd_last_error(h).decode()
        t = (C.c_double * 4)()
        assert lib.gd_cnveval_timing(h, t, 4) == 0
        runs.append(dict(wall_s=round(wall, 6), upload_s=round(t[0], 6), kernels_s=round(t[1], 6), readback_s=round(t[2], 6),
                         positive_kernel_s=round(t[3], 6), pairs_kernel_s=round(t[1] - t[3], 6)))
        totals.append(stats.sum(axis=0).tolist())
    lib.gd_destroy(h)
    assert all(t == totals[0] for t in totals), "the totals of two runs differ"
    res["cold"], res["warm"] = runs[0], runs[1:]
    kern = float(np.median([r["kernels_s"] for r in runs[1:]]))
    res["warm_median"] = {k: float(np.median([r[k] for r in runs[1:]])) for k in runs[0]}
    res["pairs_per_s_kernels"] = res["pairs"] / kern if kern > 0 else None
    res["totals_class_by_fp_fn_tp_tn"] = totals[0]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
