"""`goleft-depth index`: a BAM's .bai as htslib's indexer writes it, or its .csi (csi=True: for references beyond 2^29),
made on the device (DESIGN.md sections 3.19 and 3.20)."""
from __future__ import annotations

import ctypes as C
import os

from . import _hostlib

STATUS = {-1: "GD_E_INVALID", -2: "GD_E_NOMEM", -3: "GD_E_HIP", -4: "GD_E_STATE", -5: "GD_E_RANGE", -6: "GD_E_NODEVICE",
          -7: "GD_E_UNSORTED", -8: "GD_E_CAPACITY"}


class Refused(Exception):
    """The file was refused: `status` is the library's (GD_E_UNSORTED, GD_E_INVALID, ...)."""

    def __init__(self, status, message):
        super().__init__("%s: %s" % (STATUS.get(status, status), message))
        self.status = status


def build_stats(path: str, csi: bool = False, min_shift: int = 14):
    """(the .bai's bytes, {"records", "rounds", "ranges"}) of the BAM at `path`; rounds: walks that repaired a wrong guess.
    csi: the .csi's bytes (BGZF) with bins of 2^min_shift positions at the deepest level (8 to 24), and "min_shift" and
    "depth" among the stats."""
    lib = _hostlib.load()
    out, n = C.c_void_p(), C.c_size_t()
    stats = (C.c_int64 * 5)()
    err = C.create_string_buffer(1024)
    if csi:
        rc = lib.gdh_index_build_csi(os.fsencode(path), 1, min_shift, C.byref(out), C.byref(n), stats, err, len(err))
    else:
        rc = lib.gdh_index_build(os.fsencode(path), C.byref(out), C.byref(n), stats, err, len(err))
    if rc != 0:
        raise Refused(rc, err.value.decode("utf-8", "replace"))
    try:
        st = {"records": stats[0], "rounds": stats[1], "ranges": stats[2]}
        if csi:
            st.update(min_shift=stats[3], depth=stats[4])
        return C.string_at(out, n.value), st
    finally:
        lib.gdh_index_free(out)


def build(path: str, csi: bool = False, min_shift: int = 14) -> bytes:
    """The .bai of the BAM at `path`, or (csi) its .csi."""
    return build_stats(path, csi, min_shift)[0]


def write(path: str, out: str | None = None, csi: bool = False, min_shift: int = 14) -> str:
    """Writes the index to `out` (default: path + ".bai", or ".csi") through a temporary file and a rename; returns where it is."""
    out = out or path + (".csi" if csi else ".bai")
    data = build(path, csi, min_shift)
    tmp = "%s.tmp.%d" % (out, os.getpid())
    try:
        with open(tmp, "wb") as fh:
            fh.write(data)
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return out
