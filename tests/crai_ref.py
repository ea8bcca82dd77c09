"""Restatement of the reference's .crai reader (indexcov/crai/crai.go; the line numbers below are that file's) in plain
Python: ReadIndex (:129-192) -- the slices of every reference of a gzip-compressed index -- and makeSizes (:56-127) -- the
slices of one reference turned into sizes per 16 384-base tile.  Everything is integer except one float64 quotient, which
Python's float computes as Go does (a product, then a division, each correctly rounded, then truncation).

Where this project deliberately stops short of the reference: a seqID below -1 or above 2^20 - 1,
|alnStart| or alnSpan above 2^31 - 1 and a sliceLen outside int32 refuse the file, and so does a gzip stream that is
damaged after its first header (the reference keeps what it had read)."""
import gzip
import re
import zlib

T = 16384                                                    # TileWidth (:43)
MAX_SEQ = (1 << 20) - 1
MAX_POS = (1 << 31) - 1
_INT = re.compile(rb"^[+-]?[0-9]+$")

PANIC_TILEWIDTH, PANIC_LOGIC = 1, 2                          # the two panics (:89, :120) as a status


class CraiError(Exception):
    """The file is refused; .line is the 1-based line of the text (0: the file cannot be opened or is not gzip)."""

    def __init__(self, line, what):
        Exception.__init__(self, "line %d: %s" % (line, what))
        self.line = line


def _atoi(tok, line, what):
    """strconv.Atoi: an optional sign and decimal digits that fit an int64."""
    if not _INT.match(tok) or not -(1 << 63) <= int(tok) < (1 << 63):
        raise CraiError(line, "unable to parse %s (%s)" % (what, tok.decode("latin1")))
    return int(tok)


def parse_text(text):
    """ReadIndex on the inflated text: per reference a list of (alnStart, alnSpan, sliceLen), in file order."""
    refs = []
    at, line = 0, 0
    while True:
        nl = text.find(b"\n", at)
        if nl < 0:
            break                                            # a last line without its newline is not seen (:135)
        ln, at, line = text[at:nl], nl + 1, line + 1
        parts = ln.strip(b" \t\n\v\f\r").split(b"\t")
        if len(parts) != 6:
            raise CraiError(line, "expected 6 fields in index, got %d" % len(parts))
        si = _atoi(parts[0], line, "seqID")
        if si == -1:
            continue                                         # unmapped (:145-148): the other fields are not looked at
        if si < -1 or si > MAX_SEQ:
            raise CraiError(line, "seqID %d is outside 0 .. 2^20 - 1" % si)
        while len(refs) <= si:
            refs.append([])
        start = _atoi(parts[1], line, "alignment start")
        if abs(start) > MAX_POS:
            raise CraiError(line, "alignment start %d is outside +-(2^31 - 1)" % start)
        span = _atoi(parts[2], line, "alignment span")
        if span < 0:
            break                                            # (:163-166) what was read so far is kept
        if span > MAX_POS:
            raise CraiError(line, "alignment span %d is above 2^31 - 1" % span)
        _atoi(parts[3], line, "container start")
        _atoi(parts[4], line, "slice start")
        ln_ = _atoi(parts[5], line, "slice length")
        if not -(1 << 31) <= ln_ < (1 << 31):
            raise CraiError(line, "slice length %d is outside int32" % ln_)
        refs[si].append((start, span, ln_))
    return refs


def read_index(path):
    try:
        with open(path, "rb") as f:
            raw = f.read()
        text = gzip.decompress(raw)                          # every member of the file, one after the other
    except (OSError, EOFError, zlib.error) as e:
        raise CraiError(0, "not a gzip file: %s" % e)
    return parse_text(text)


def make_sizes(slices, stats=None):
    """makeSizes: (sizes, status).  stats: a dict that counts shifts, skipped and small slices."""
    sizes = []
    last_val = 0
    for start, span, slen in slices:
        last_start = T * len(sizes)
        k = 0
        while last_start < start - T:                        # back fill gaps (:78-86)
            sizes.append(last_val if k == 0 else 0)
            last_val = 0 if k == 0 else last_val
            last_start += T
            k += 1
        if start - last_start > T:
            return sizes, PANIC_TILEWIDTH
        while start - last_start < -T:                       # a long read of the slice before reaches into this one
            start += T
            span -= T
            if stats is not None:
                stats["shifts"] = stats.get("shifts", 0) + 1
        if span <= 0:
            if stats is not None:
                stats["skipped"] = stats.get("skipped", 0) + 1
            continue
        q = 100000 * float(slen) / float(span)
        per_base = int(q)                                    # truncation towards zero
        n_tiles = span >> 14
        if n_tiles == 0 and start - last_start < T:
            last_val = per_base
            if stats is not None:
                stats["small"] = stats.get("small", 0) + 1
            continue
        sizes.extend([per_base] * n_tiles)
        s = start + span
        cmp_ = -((-s) // T) if s < 0 else s // T             # Go's integer division truncates
        if len(sizes) > cmp_ + 1 or cmp_ < len(sizes) - 1:
            return sizes, PANIC_LOGIC
        last_val = per_base
    return sizes, 0


def index_sizes(path):
    """Index.Sizes (:45-51): per reference the tile sizes.  A panic of makeSizes is a CraiError here."""
    out = []
    for r, sl in enumerate(read_index(path)):
        sizes, status = make_sizes(sl)
        if status:
            raise CraiError(0, "reference %d: makeSizes panics (%d)" % (r, status))
        out.append(sizes)
    return out
