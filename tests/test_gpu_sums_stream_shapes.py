"""-m gpu: gd_sums_stream_kernel and its fallback gd_tile_sums_kernel at the streaming kernel's structural edges --
read counts around 256 / 768 / 4096, more than 64 contigs, the per-wave queue exactly full and one past full, reads
that end on the end of a lane's third window, the 257th window of a wave, the 2^22-base bound, window sizes near 2^31.
The shapes come from tests/sums_shapes.py; tests/test_sums_shapes.py shows on the CPU that each one reaches its edge.

Every contig's window sums (empty contigs included) must equal the C oracle's exactly, under both kernels; on a contig
too long for a per-base vector the interval reference stands in.  No tolerance anywhere: integer equality."""
import numpy as np
import pytest

from tests import sums_shapes as S

pytestmark = pytest.mark.gpu


def same(got, want, ctx, tid, W):
    """None when equal; else a message that names the contig, the first window that differs and both values."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    n = min(len(got), len(want))
    neq = np.flatnonzero(got[:n] != want[:n])
    k = int(neq[0]) if len(neq) else n
    return ("%s, contig %d: window %d (positions from %d) got %s, want %s; %d windows differ; %d vs %d windows"
                % (ctx, tid, k, k * W, got[k] if k < len(got) else "-", want[k] if k < len(want) else "-",
                   len(neq), len(got), len(want)))


def in_arena(r, length):
    """The records as device tensors that are the front of larger ones whose next elements look like live records:
    flag 0, MAPQ 60, one more op each -- `<length>M` at position 0.  The engine is given the front only."""
    import torch
    dev = torch.device("cuda", 0)
    n, m, extra = r.n, r.n_ops, 8
    tails = ((r.pos, np.int32, np.zeros(extra)), (r.flag, np.int16, np.zeros(extra)),
             (r.mapq, np.uint8, np.full(extra, 60)), (r.cigar_off, np.int32, m + 1 + np.arange(extra)),
             (r.cigar, np.int32, np.full(extra, length << 4)))
    out = []
    for a, dt, tail in tails:
        whole = np.concatenate([np.ascontiguousarray(a).view(dt), tail.astype(dt)])
        out.append(torch.from_numpy(whole).to(dev)[:len(a)])
    assert out[3].shape[0] == n + 1
    return out


def want_sums(name):
    c = S.case(name)
    oracle = S.oracle_sums(name)
    return [S.interval_window_sums(c.get(t), c.Q, c.flag_mask, L, c.W) if t in c.huge else oracle[t]
            for t, L in enumerate(c.lengths)]


@pytest.mark.parametrize("name", S.NAMES)
def test_window_sums_at_structural_edges(name):
    from goleft_amd import engine as E
    from goleft_amd.engine import DepthEngine
    c = S.case(name)
    want = want_sums(name)
    got = {}
    with DepthEngine(0) as eng:
        eng.set_params(window_size=c.W, min_mapq=c.Q, flag_mask=c.flag_mask)
        eng.set_path(E.PATH_TILE)
        eng.set_outputs(sums_only=True)
        eng.set_contigs(c.lengths)
        for t, r in c.reads.items():
            if c.guarded:
                eng.adopt_device(t, *in_arena(r, c.lengths[t]))
            else:
                eng.push(t, r.pos, r.flag, r.mapq, r.cigar_off, r.cigar)
        for kernel, fast, tk in (("gd_sums_stream_kernel", 1, E.TK_SUMS_STREAM_RAW), ("gd_tile_sums_kernel", 0, E.TK_TILE_SUMS)):
            eng.set_option(E.OPT_FAST_KERNEL, fast)
            eng.compute()
            assert eng.stats().tile_kernel == tk, "case %s: ran kernel %d, expected %s" % (name, eng.stats().tile_kernel, kernel)
            got[kernel] = [eng.window_sums(t) for t in range(len(c.lengths))]
    bad = []
    for kernel, sums in got.items():
        for t in range(len(c.lengths)):
            bad.append(same(sums[t], want[t], "case %s, W=%d, %s against the %s" % (
                name, c.W, kernel, "interval reference" if t in c.huge else "oracle"), t, c.W))
    # (implied by the two comparisons above; kept so that a failure says which kernel moved)
    for t in range(len(c.lengths)):
        bad.append(same(got["gd_sums_stream_kernel"][t], got["gd_tile_sums_kernel"][t],
                        "case %s, W=%d, gd_sums_stream_kernel against gd_tile_sums_kernel" % (name, c.W), t, c.W))
    bad = [b for b in bad if b]
    assert not bad, "%d comparisons differ:\n%s" % (len(bad), "\n".join(bad[:12]))
