"""A restatement of dcnv's ChunkDebiaser (dcnv/debiaser/debiaser.go:125-171 of the reference, with the Sort and Unsort of
:56-93 around it) in plain Python / numpy: what gd_chunk_debias, `goleft-depth debias` and `emdepth --gc-values` are held
to, bit for bit.

Sort (:56-76) orders the rows by Vals ascending; Debias (:133-171) then walks the SORTED vals:

  chunks (:140-148)   slices = [0], v0 = sorted[0]; for every i, `sorted[i] - v0 > W` (a float64 subtraction, strictly
                      greater) sets v0 = sorted[i] and appends i; R is appended at the end.  A row's chunk is the slice
                      its sorted position falls in.  A boundary needs a strictly positive difference, so it never falls
                      between two equal values: which of the tied rows the argsort puts first changes nothing.
  "median" (:153-161) of the n cells a sample has in a chunk: sort ascending, k = the leading values equal to 0 (-0.0
                      compares equal and counts), median = sorted[(n - k) / 2] by integer division -- the index counts
                      from the START of the chunk, not from k, so a chunk with n < 3k has median 0.
  division (:163-167) when the median is > 0 every cell of the chunk becomes d / median in float64; otherwise the chunk
                      of that sample is left as it is.

Unsort (:79-93) puts the rows back, so nothing of the order is left in the result: inside a chunk only the SET of rows
matters.  This project's matrices are float32: the cells are widened, the division is one float64 division, and both the
float64 quotient and its float32 narrowing are returned.  A median that is a zero is reported as +0.0."""
import numpy as np


def chunks(vals, window, order=None):
    """(order [R], slices [C + 1], chunk_of_row uint32 [R]); order: an argsort of vals, any order among ties"""
    vals = np.asarray(vals, np.float64)
    W = np.float64(window)
    assert vals.ndim == 1 and len(vals) >= 1 and np.all(np.isfinite(vals)) and np.isfinite(W) and W > 0
    if order is None:
        order = np.argsort(vals, kind="stable")
    order = np.asarray(order, np.int64)
    s = vals[order]
    assert np.all(s[1:] >= s[:-1])
    slices = [0]                                 # :140
    v0 = s[0]                                    # :141
    for i in range(len(s)):                      # :142
        if s[i] - v0 > W:                        # :143
            v0 = s[i]                            # :144
            slices.append(i)                     # :145
    slices.append(len(s))                        # :148
    chunk_of_row = np.zeros(len(s), np.uint32)
    for c in range(len(slices) - 1):
        chunk_of_row[order[slices[c]:slices[c + 1]]] = c
    return order, np.array(slices, np.int64), chunk_of_row


def chunk_median(cells):
    """sorted[(n - k) / 2] of one sample's cells in one chunk (:155-161), of the cells' type"""
    s = np.sort(np.asarray(cells), kind="stable")          # :157
    k = 0
    while k < len(s) and s[k] == 0:              # :159
        k += 1
    m = s[(len(s) - k) // 2]                     # :161
    return m if m != 0 else s.dtype.type(0)


def debias(matrix, vals, window, order=None):
    """(out64 float64 [R][N], out float32 [R][N], chunk_of_row uint32 [R], n_chunks, med float32 [C][N])"""
    m = np.asarray(matrix, np.float32)
    assert m.ndim == 2 and m.shape[0] == len(vals) and np.all(np.isfinite(m)) and np.all(m >= 0)
    order, slices, chunk_of_row = chunks(vals, window, order)
    C = len(slices) - 1
    out64 = m.astype(np.float64)
    med = np.zeros((C, m.shape[1]), np.float32)
    with np.errstate(over="ignore"):
        for c in range(C):
            rows = order[slices[c]:slices[c + 1]]
            for s in range(m.shape[1]):              # :151
                med[c, s] = chunk_median(m[rows, s])
                if med[c, s] > 0:                    # :163
                    out64[rows, s] = m[rows, s].astype(np.float64) / np.float64(med[c, s])      # :165
        out = out64.astype(np.float32)
    return out64, out, chunk_of_row, C, med


def matrix_text(header, where, out):
    """what `goleft-depth debias` writes: the header, and per row its `chrom start end` and %.9g of each float32"""
    lines = [header]
    for w, row in zip(where, np.asarray(out, np.float32)):
        lines.append("\t".join([w] + ["%.9g" % float(v) for v in row]))
    return "\n".join(lines) + "\n"
