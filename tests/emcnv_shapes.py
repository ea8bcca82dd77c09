"""The matrices the emcnv tests run, seeded, with their restatement results computed once a process.

CPU tests (tests/test_emcnv_ref.py) assert on every case, from the restatement alone: no cell within 1e-9 of a state
threshold, no row emdepth_shapes.plan would leave out, at most 1 % of member cells excluded by pair_excluded, and at
least one CNV where one is meant.  The GPU tests (tests/test_gpu_emcnv.py) run the same cases through the C ABI.

Shapes follow the kernels (goleft_amd/csrc/gd_emcnv.hpp): 64 samples a member word, columns walked in chunks of CHUNK
rows, one wavefront a row and WAVES rows a workgroup in the per-block kernels, at most GRID workgroups a launch: their
stride turns at GRID * WAVES rows (the 'rows_stride' case).  The kernels of gd_emcnv_finish have no stride loop: their
grids cover the rows, the (chunk, word) pairs and the CNVs.  The gap kernel steps over blocks of SPAN1 and SPAN2 rows
whose starts all lie inside its window (the 'repeated_long', 'near_long' and 'repeated_wrap' cases), and the members
kernel takes 64 rows of a CNV a step ('long_cnv', 'dense', 'sparse_long')."""
import functools

import numpy as np

from tests import emcnv_ref as C
from tests import emdepth_ref as R
from tests import emdepth_shapes as ES

CHUNK = 256              # rows of a column chunk (EMCNV_CHUNK)
WAVES = 4                # rows of a workgroup of the per-block kernels (EMCNV_WAVES)
GRID = 2048              # workgroups of a launch of the per-block kernels at most (EMCNV_MAX_GRID)
SPAN1, SPAN2 = 64, 4096  # rows of the blocks the gap kernel may step over
SAMPLE_COUNTS = (1, 3, 4, 63, 64, 65, 256, 257)
BLOCKS = (1, 2, 7, None)                         # block seams: rows per gd_emcnv_add (None: all)
UP, DOWN, ZERO = 80.0, 20.0, 0.0                 # against a level of 36 .. 44: log2fc about +1, -1, -Inf
CAP = 0.01


class Case:
    def __init__(self, depths, starts, ends, want=True, exact=True, kind="f32", cells=None, scale=None):
        self.depths = np.ascontiguousarray(depths, np.float32)
        self.starts = np.ascontiguousarray(np.asarray(starts, np.int64) & 0xFFFFFFFF, np.uint32)
        self.ends = np.ascontiguousarray(np.asarray(ends, np.int64) & 0xFFFFFFFF, np.uint32)
        assert self.starts.shape == self.ends.shape == (self.depths.shape[0],)
        self.want, self.exact, self.kind, self.cells, self.scale = want, exact, kind, cells, scale


def level(seed, rows, n):
    """integers 36 .. 44: every sum over a bin is exact in float64 in any order"""
    return np.random.default_rng(seed).integers(36, 45, size=(rows, n)).astype(np.float32)


def tiled(rows, width=10000, first=1000000, jumps=()):
    """back-to-back rows of one width; a jump (row, by) moves that row and all after it"""
    st = first + np.arange(rows, dtype=np.int64) * width
    for r, by in jumps:
        st[r:] += by
    return st, st + width


def put(d, events):
    """events: (first row, row after the last, sample, depth)"""
    for r0, r1, s, v in events:
        d[r0:r1, s] = v
    return d


def simple(seed, rows, n, events, want=True, **pos):
    st, en = tiled(rows, **pos)
    return Case(put(level(seed, rows, n), events), st, en, want)


def gap_case(g):
    """members of rows 2, 3 and of rows 6, 7 of sample 1; every row from 4 on starts g past the end of row 3 and
    has no width, so row 3 sees the same distance from all of them and they see none among themselves"""
    d = put(level(40, 10, 5), [(1, 4, 1, UP), (5, 8, 1, UP)])
    st, en = tiled(10, width=1000)
    st[4:] = en[3] + g
    en[4:] = st[4:]
    return Case(d, st, en)


def final_case(width):
    d = put(level(41, 8, 5), [(4, 8, 2, DOWN)])
    st, en = tiled(8, width=1000)
    en[7] = st[7] + width
    return Case(d, st, en, want=width <= 70000)


def random_case(seed, rows, n):
    """events in a quarter of the columns (so a row's centre stays the level's), positions with jumps forward and
    one restart (another chromosome)"""
    rng = np.random.default_rng(seed)
    d = level(seed + 1, rows, n)
    cols = rng.choice(n, size=max(1, n // 4), replace=False)
    for _ in range(max(3, rows * len(cols) // 12)):
        r0 = int(rng.integers(0, rows))
        d[r0:r0 + int(rng.integers(2, 7)), rng.choice(cols)] = rng.choice([UP, UP, DOWN, DOWN, ZERO])
    jumps = [(int(r), 50000) for r in rng.choice(np.arange(1, max(2, rows)), size=max(1, rows // 10), replace=False)] if rows > 1 else []
    st, en = tiled(rows, width=int(rng.choice([1000, 5000, 10000])), jumps=jumps)
    width = en - st
    if rows > 8:
        st[rows // 2:] -= st[rows // 2] - 500    # the second half restarts at 500: another chromosome
    return Case(d, st, st + width, want=None)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    # rows 0, 1, 2
    c["rows_0"] = Case(np.zeros((0, 5), np.float32), [], [], want=False)
    c["rows_1_zero"] = Case(np.zeros((1, 5), np.float32), [100], [200])                      # row 0 against itself: all D
    c["rows_1_plain"] = Case(level(1, 1, 5), [100], [200], want=False)
    c["rows_2"] = simple(2, 2, 5, [(0, 2, 3, UP)])
    # states
    c["u_run"] = simple(3, 12, 5, [(2, 7, 2, UP)])
    c["d_run"] = simple(4, 12, 5, [(2, 7, 2, DOWN)])
    c["u_to_d"] = simple(5, 14, 5, [(2, 6, 2, UP), (6, 10, 2, DOWN)])
    c["n_between"] = simple(6, 14, 5, [(2, 5, 2, UP), (6, 9, 2, UP)])
    c["zero_cell"] = simple(7, 12, 5, [(2, 6, 3, ZERO)])
    c["zero_rows"] = simple(8, 12, 5, [(4, 5, s, ZERO) for s in range(5)] + [(8, 10, s, ZERO) for s in range(5)])
    fb = level(9, 12, 4)
    fb[3:8] = [0, 0, 1, 1000]                                                                # bin 2 empty: the fallback moves lambda[2]
    c["fallback"] = Case(fb, *tiled(12))
    # gaps, wraps, the final test
    for g in (29999, 30000, 30001):
        c["gap_%d" % g] = gap_case(g)
    c["start_before_end"] = simple(10, 12, 5, [(2, 9, 1, UP)], jumps=[(6, -1040000)])          # row 6 starts at 20000: a wrap is a gap
    c["final_wrap"] = simple(11, 8, 5, [(3, 8, 1, UP)], width=1000, first=2 ** 32 - 100000 - 5000)
    c["final_wrap_past"] = simple(12, 8, 5, [(3, 8, 1, UP)], width=1000, first=2 ** 32 - 6500, want=None)     # the positions themselves wrap
    for w in (70000, 70001):
        c["final_%d" % w] = final_case(w)
    rep = put(level(13, 10, 5), [(2, 8, 1, UP), (3, 6, 2, DOWN)])
    c["repeated"] = Case(rep, [5000] * 10, [5000] * 10)                                      # F never fires before the end
    # sample 0: runs of 1 and 3 members, a gap next or not
    c["sample0"] = simple(14, 24, 5, [(1, 3, 0, UP), (5, 7, 0, UP), (9, 13, 0, DOWN), (15, 19, 0, DOWN), (22, 24, 0, UP),
                                      (9, 13, 3, UP)],
                          width=1000, jumps=[(7, 50000), (13, 50000)])
    one = np.full((14, 1), 40.0, np.float32)
    one[[2, 3, 6, 7, 8, 11, 12, 13], 0] = 0.0
    c["one_sample"] = Case(one, *tiled(14, width=1000, jumps=[(4, 50000), (8, 50000)]))
    # PSize: 1, several, and four of nine samples pending at once
    c["psize"] = simple(15, 30, 9, [(2, 7, 1, UP), (12, 18, 2, UP), (13, 19, 3, DOWN), (12, 15, 5, UP)] +
                        [(22, 27, s, DOWN) for s in (1, 2, 3, 4)], jumps=[(9, 50000), (20, 50000)])
    # structure: the chunk and its neighbours, a CNV longer than a chunk, many CNVs at one row, dense, none
    for rows in (CHUNK - 1, CHUNK, CHUNK + 1):
        c["rows_%d" % rows] = simple(16 + rows, rows, 5, [(rows - 6, rows, 1, UP), (CHUNK // 2, CHUNK // 2 + 5, 2, DOWN), (0, 3, 3, UP)],
                                     width=1000, jumps=[(CHUNK // 2 + 20, 50000)])
    c["long_cnv"] = simple(17, 2 * CHUNK + 10, 5, [(5, 2 * CHUNK + 4, 1, UP), (CHUNK - 3, CHUNK + 3, 2, DOWN)], width=1000)
    c["many_at_one_row"] = simple(18, 12, 65, [(2, 6, s, UP if s & 1 else DOWN) for s in range(1, 31)], jumps=[(8, 50000)])
    c["dense"] = simple(19, 2 * CHUNK + 44, 64, [(0, 2 * CHUNK + 44, s, UP) for s in range(0, 60, 2)], width=1000,
                        jumps=[(r, 50000) for r in range(40, 2 * CHUNK, 90)])
    c["no_members"] = simple(20, 20, 5, [], want=False)
    # rows that never gap, over more than two blocks of SPAN2 rows: all at one position, at one position whose window
    # wraps past 2^32, and scattered inside 20 000 positions (no width: a start below an end wraps into a gap)
    rows = 2 * SPAN2 + SPAN1 + 6
    ev = [(3, 40, 1, UP), (SPAN1 - 2, SPAN1 + 3, 2, DOWN), (SPAN2 - 3, SPAN2 + 3, 1, DOWN), (rows - 9, rows, 2, UP), (100, 103, 0, UP)]
    c["repeated_long"] = Case(put(level(22, rows, 3), ev), [5000] * rows, [5000] * rows)
    c["repeated_wrap"] = Case(put(level(23, rows, 3), ev), [2 ** 32 - 10000] * rows, [2 ** 32 - 10000] * rows)
    near = 5000 + (np.arange(rows, dtype=np.int64) * 7919) % 20000
    near[SPAN2 + 77] += 40000                                                                # one row outside every window
    c["near_long"] = Case(put(level(24, rows, 3), ev), near, near)
    # one CNV of few members spread over many rows (a member every 25 rows, no gap between them)
    sp = level(25, 40 * 25 + 2, 5)
    for r0 in range(0, 40 * 25, 25):
        sp[r0:r0 + 2, 3] = UP
    c["sparse_long"] = Case(sp, *tiled(40 * 25 + 2, width=1000))
    c["rows_stride"] = simple(21, GRID * WAVES + 5, 3, [(GRID * WAVES - 3, GRID * WAVES + 5, 1, UP), (10, 14, 2, DOWN)],
                              width=1000)
    for n in SAMPLE_COUNTS:
        if n > 1:
            c["random_n%d" % n] = random_case(100 + n, 12 if n > 200 else 40, n)
    # one general float32 matrix: a level per row, a factor per event, 5 % noise
    rng = np.random.default_rng(300)
    f = put(np.ones((40, 200)), [(int(r0), int(r0) + 5, int(s), v) for r0, s, v in
                                 zip(rng.integers(0, 36, 60), rng.integers(0, 200, 60), rng.choice([2.0, 0.5, 0.0], 60))])
    g = (rng.uniform(20.0, 60.0, size=(40, 1)) * f * rng.lognormal(0.0, 0.05, size=(40, 200))).astype(np.float32)
    c["float_n200"] = Case(g, *tiled(40, width=5000, jumps=[(17, 80000)]), exact=False)
    # the cells form on what a real gd_depthwed_device leaves (the cohort of the emdepth tests)
    for n in ES.COHORT_SAMPLES:
        cells = ES.cohort(n)[1]
        st = np.concatenate([np.arange((L + ES.COHORT_W - 1) // ES.COHORT_W, dtype=np.int64) * ES.COHORT_W for L in ES.COHORT_LENGTHS])
        en = np.concatenate([np.minimum(np.arange((L + ES.COHORT_W - 1) // ES.COHORT_W, dtype=np.int64) * ES.COHORT_W + ES.COHORT_W, L)
                             for L in ES.COHORT_LENGTHS])
        c["cohort_n%d" % n] = Case(R.cells_to_depths(cells), st, en, want=None, kind="cohort", cells=cells)
        sc = ES.pow2_scales(610 + n, n)
        c["cohort_pow2_n%d" % n] = Case(R.cells_to_depths(cells, sc), st, en, want=None, kind="cohort", cells=cells, scale=sc)
    return c


_EM_CACHE = {}


def em_rows(depths):
    """emdepth_ref.em_matrix, a row seen before not computed again."""
    out = []
    for row in np.ascontiguousarray(depths, np.float32):
        k = row.tobytes()
        if k not in _EM_CACHE:
            _EM_CACHE[k] = R.em_row(row)
        out.append(_EM_CACHE[k])
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's result of a case, computed once and not changed."""
    case = cases()[name]
    return C.run(case.depths, case.starts, case.ends, em_rows(case.depths))


def plan(name):
    """(rows emdepth_shapes.plan leaves out, member cells, member cells pair_excluded leaves out as a set of (row, sample))"""
    case, ref = cases()[name], reference(name)
    keep, out, _ = ES.plan(case, ref.rows)
    members = {(r, cnv.sample) for cnv in ref.cnvs for r in cnv.rows}
    return int((~keep).sum()) if len(keep) else 0, members, out & members


def flatten(cnvs):
    """The arrays gd_emcnv_read gives, from the restatement's CNVs."""
    off = np.zeros(len(cnvs) + 1, np.uint64)
    off[1:] = np.cumsum([len(c.rows) for c in cnvs], dtype=np.uint64)
    cat = lambda key, dt: np.array([v for c in cnvs for v in getattr(c, key)], dt)
    return dict(sample=np.array([c.sample for c in cnvs], np.uint32), psize=np.array([c.psize for c in cnvs], np.uint32),
                emit_row=np.array([c.emit_row for c in cnvs], np.uint32), member_off=off,
                member_row=cat("rows", np.uint32), depth=cat("depth", np.float32), cn=cat("cn", np.uint8),
                log2fc=cat("log2fc", np.float32))


CLI_SCALES = ES.CLI_SCALES                       # as the --scales file spells them
CLI_NAMES = tuple("s%d" % i for i in range(9))


def cli_cells():
    """The 9-sample, 40-row integer matrix of the command-line tests: 25 rows of chr1, 15 of chr2 (whose first row
    starts before the end of chr1's last: a gap), calls that end at the boundary, one that the boundary cuts, a run of
    depth 0 (log2fc -Inf), and one-site calls of sample 0."""
    d = put(level(500, 40, 9), [(3, 10, 1, UP), (5, 13, 4, DOWN), (20, 27, 0, UP), (22, 29, 2, UP), (30, 34, 7, ZERO),
                                (32, 40, 5, DOWN)])
    return d.astype(np.int64)


def cli_where():
    """(chrom, start, end) of every row"""
    return [("chr%d" % (1 + i // 25), (i % 25) * 1000, (i % 25 + 1) * 1000) for i in range(40)]


@functools.lru_cache(maxsize=None)
def cli_reference(scaled):
    cells = cli_cells()
    depths = R.cells_to_depths(cells, np.array(CLI_SCALES, np.float32) if scaled else None)
    return C.run(depths, [w[1] for w in cli_where()], [w[2] for w in cli_where()], em_rows(depths))


def cli_text(res):
    """The --cnvs file of a restatement result."""
    where = cli_where()
    fc = lambda v: ("+Inf" if v > 0 else "-Inf") if np.isinf(v) else "%.2f" % float(v)
    lines = ["#sample\tindex\tpsize\tsites\tpositions\tcn\tdepth\tlog2fc"]
    for c in res.cnvs:
        lines.append("\t".join([CLI_NAMES[c.sample], str(c.sample), str(c.psize), str(len(c.rows)),
                                ",".join("%s:%d-%d" % where[r] for r in c.rows), ",".join(str(v) for v in c.cn),
                                ",".join("%.9g" % float(v) for v in c.depth), ",".join(fc(v) for v in c.log2fc)]))
    return "\n".join(lines) + "\n"
