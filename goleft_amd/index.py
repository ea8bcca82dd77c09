"""`goleft-depth index`: a BAM's .bai as htslib's indexer writes it, made on the device."""
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


def build_stats(path: str):
    """(the .bai's bytes, {"records", "rounds", "ranges"}) of the BAM at `path`; rounds: walks that repaired a wrong guess."""
    lib = _hostlib.load()
    out, n = C.c_void_p(), C.c_size_t()
    stats = (C.c_int64 * 3)()
    err = C.create_string_buffer(1024)
    rc = lib.gdh_index_build(os.fsencode(path), C.byref(out), C.byref(n), stats, err, len(err))
    if rc != 0:
        raise Refused(rc, err.value.decode("utf-8", "replace"))
    try:
        return C.string_at(out, n.value), {"records": stats[0], "rounds": stats[1], "ranges": stats[2]}
    finally:
        lib.gdh_index_free(out)


def build(path: str) -> bytes:
    """The .bai of the BAM at `path`."""
    return build_stats(path)[0]


def write(path: str, out: str | None = None) -> str:
    """Writes the index to `out` (default: path + ".bai") through a temporary file and a rename; returns where it is."""
    out = out or path + ".bai"
    data = build(path)
    tmp = "%s.tmp.%d" % (out, os.getpid())
    try:
        with open(tmp, "wb") as fh:
            fh.write(data)
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return out
