"""Generate tests/golden/lz4_craft.json: what liblz4 1.9.3 and the compiled
reference reader make of every hand-built frame of tests/lz4_craft.py's CASES.

Run in the build container (needs /opt/conda's liblz4 1.9.3 and oracle/_ref
built by `make -C oracle ref`):

    python tests/golden/make_lz4_craft.py

For every case it records
  * liblz4's verdict on the frame alone: LZ4F_decompress of the whole frame
    into a buffer of LZ4F_CAP bytes (more than any case decodes, so every
    block is decoded in place) -- accepted or not, the error name, the decoded
    length and the SHA-256 of the decoded bytes;
  * the compiled REFERENCE reader's answers (oracle/_ref) on a seekable file
    that holds the frame between two intact neighbours: a caller's loop of
    zseek_pread (test/example.c) with cache 0 and 1 -- bytes delivered, their
    SHA-256, the last return value and its error string.  Each case runs in a
    child process with a time limit, since the reference can spin on a frame
    that ends early; such a case is recorded as "hang".

Only data is written (names, numbers, hashes, strings).  The frames themselves
are regenerated from lz4_craft.CASES; "frame_sha" pins them, so a changed
table without a regenerated record fails test_lz4_craft.py.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import select
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lz4_craft  # noqa: E402
from oracle.oracle import RefZseek  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
LZ4_SO = "/opt/conda/lib/liblz4.so.1.9.3"
LZ4F_CAP = 2 << 20
HANG_SECONDS = 20


def sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


def load_lz4():
    if not os.path.exists(LZ4_SO):
        return None
    lz = C.CDLL(LZ4_SO)
    lz.LZ4_versionNumber.restype = C.c_int
    lz.LZ4F_createDecompressionContext.restype = C.c_size_t
    lz.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    lz.LZ4F_freeDecompressionContext.restype = C.c_size_t
    lz.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
    lz.LZ4F_decompress.restype = C.c_size_t
    lz.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p,
                                   C.POINTER(C.c_size_t), C.c_void_p]
    lz.LZ4F_isError.restype = C.c_uint
    lz.LZ4F_isError.argtypes = [C.c_size_t]
    lz.LZ4F_getErrorName.restype = C.c_char_p
    lz.LZ4F_getErrorName.argtypes = [C.c_size_t]
    return lz


def lz4f_decode(lz, frame: bytes, cap: int = LZ4F_CAP):
    """LZ4F_decompress until the frame ends, fails or stops moving ->
    (error name or "" or "stalled", decoded bytes)"""
    ctx = C.c_void_p()
    assert not lz.LZ4F_isError(lz.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    src = C.create_string_buffer(frame, len(frame))
    dst = C.create_string_buffer(cap)
    sp = dp = 0
    try:
        while True:
            ds, ss = C.c_size_t(cap - dp), C.c_size_t(len(frame) - sp)
            r = lz.LZ4F_decompress(ctx, C.addressof(dst) + dp, C.byref(ds), C.addressof(src) + sp, C.byref(ss), None)
            if lz.LZ4F_isError(r):
                return lz.LZ4F_getErrorName(r).decode(), dst.raw[:dp]
            dp += ds.value
            sp += ss.value
            if r == 0:
                return "", dst.raw[:dp]
            if ds.value == 0 and ss.value == 0:
                return "stalled", dst.raw[:dp]
    finally:
        lz.LZ4F_freeDecompressionContext(ctx)


def case_image(frame: bytes, dsize: int):
    """the case between its two intact neighbours -> (seekable file, decoded size)"""
    (fa, a), (fb, b) = lz4_craft.NEIGHBOURS
    return lz4_craft.seekable([fa, frame, fb], [len(a), dsize, len(b)]), len(a) + dsize + len(b)


def pread_loop(pread, total: int):
    """a caller's loop (test/example.c): zseek_pread from where the last call
    ended until it returns <= 0 -> (bytes delivered, the last return value)"""
    got, pos = b"", 0
    while True:
        rv, b = pread(total - pos if total > pos else 1, pos)
        if rv <= 0:
            return got, int(rv)
        got += b
        pos += rv


def ref_answers(ref, img: bytes, total: int):
    out = {}
    for cache in (0, 1):
        r = ref.open(img, cache)
        got, rv = pread_loop(r.pread, total)
        out[f"cache{cache}"] = {"bytes": len(got), "sha": sha(got), "last": rv, "error": r.error if rv < 0 else ""}
        r.close()
    return out


def ref_answers_guarded(ref, img: bytes, total: int):
    """ref_answers in a child process; "hang" if it does not end"""
    rd, wr = os.pipe()
    pid = os.fork()
    if pid == 0:
        os.close(rd)
        try:
            os.write(wr, json.dumps(ref_answers(ref, img, total)).encode())
        finally:
            os._exit(0)
    os.close(wr)
    ready, _, _ = select.select([rd], [], [], HANG_SECONDS)
    if not ready:
        os.kill(pid, signal.SIGKILL)
    data = b""
    while ready:
        chunk = os.read(rd, 65536)
        if not chunk:
            break
        data += chunk
    os.close(rd)
    os.waitpid(pid, 0)
    return json.loads(data) if data else "hang"


def main():
    lz = load_lz4()
    assert lz is not None and lz.LZ4_versionNumber() == 10903, "liblz4 1.9.3 missing"
    ref = RefZseek()
    assert ref.versions["lz4"] == 10903, ref.versions
    cases = []
    for name, frame, dsize, want in lz4_craft.CASES:
        err, got = lz4f_decode(lz, frame)
        img, total = case_image(frame, dsize)
        cases.append({"name": name, "frame_sha": sha(frame), "dsize": dsize,
                      "lz4f": {"ok": err == "", "error": err, "len": len(got), "sha": sha(got) if err == "" else ""},
                      "reference": ref_answers_guarded(ref, img, total)})
    with open(os.path.join(OUT, "lz4_craft.json"), "w") as f:
        json.dump({"lz4f_cap": LZ4F_CAP, "neighbour_frame_shas": [sha(f) for f, _ in lz4_craft.NEIGHBOURS],
                   "cases": cases}, f, indent=1)
    print(len(cases), "cases;", sum(c["lz4f"]["ok"] for c in cases), "accepted by LZ4F_decompress alone;",
          sum(c["reference"] == "hang" for c in cases), "hang the reference reader")


if __name__ == "__main__":
    main()
