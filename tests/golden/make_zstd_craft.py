"""Generate tests/golden/zstd_craft.json: what libzstd 1.4.9 and the compiled
reference reader make of every hand-built entry of tests/zstd_craft.py's CASES.

Run in the build container (needs /opt/conda's libzstd 1.4.9 and oracle/_ref
built by `make -C oracle ref`):

    python tests/golden/make_zstd_craft.py

For every case it records
  * the SHA-256 of the entry and its declared size;
  * libzstd's verdict on the entry alone: ZSTD_decompressDCtx into a buffer of
    the declared size -- its error code (0: none), the decoded length and the
    SHA-256 of the decoded bytes;
  * the compiled REFERENCE reader's answers (oracle/_ref) on a seekable file
    that holds the entry between two intact neighbours: a caller's loop of
    zseek_pread (test/example.c) with cache 0 and 1 -- bytes delivered, their
    SHA-256, the last return value and its error string.  Each case runs in a
    child process with a time limit, since the reference can spin on an entry
    that decodes short; such a case is recorded as "hang".

Only data is written (names, numbers, hashes, strings).  Hashes and error
texts are kept once, in "strings", and referred to by index; a case is the list
[name, entry sha, d_size, code, decoded length, decoded sha, reference], the
reference "hang" or per cache [bytes, sha, last return value, error text].
The entries themselves are regenerated from zstd_craft.CASES; the entry hash
pins them, so a changed table without a regenerated record fails
test_zstd_craft.py.
"""
from __future__ import annotations

import hashlib
import json
import os
import select
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zstd_craft  # noqa: E402
import zstd_util  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
HANG_SECONDS = 20


def sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


def load_zstd():
    z = zstd_util.load()
    if z is None:
        return None
    z.ZSTD_versionNumber.restype = zstd_util.C.c_uint
    return z if z.ZSTD_versionNumber() == 10409 else None


def libzstd_answer(z, entry: bytes, dsize: int):
    """-> [error code, decoded length, SHA-256 of the decoded bytes or ""]"""
    got, code = zstd_util.decode(z, entry, dsize)
    return [int(code), len(got), sha(got) if code == 0 else ""]


def case_image(entry: bytes, dsize: int, around: int = 1):
    """the case between its intact neighbours (`around` of them on each side,
    the two kinds taking turns) -> (seekable file, the sizes of its entries)"""
    nb = zstd_craft.NEIGHBOURS
    before = [nb[i % 2] for i in range(around)]
    after = [nb[(i + 1) % 2] for i in range(around)]
    frames = [f for f, _ in before] + [entry] + [f for f, _ in after]
    sizes = [len(c) for _, c in before] + [dsize] + [len(c) for _, c in after]
    return zstd_craft.seekable(frames, sizes), sizes


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
    out = []
    for cache in (0, 1):
        r = ref.open(img, cache)
        got, rv = pread_loop(r.pread, total)
        out.append([len(got), sha(got), rv, r.error if rv < 0 else ""])
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


class Pool:
    def __init__(self, strings=None):
        self.strings = list(strings or [])
        self.index = {s: i for i, s in enumerate(self.strings)}

    def put(self, s: str) -> int:
        if s not in self.index:
            self.index[s] = len(self.strings)
            self.strings.append(s)
        return self.index[s]


def pack(pool: Pool, name, entry, dsize, lib, ref):
    if ref != "hang":
        ref = [[n, pool.put(h), rv, pool.put(err)] for n, h, rv, err in ref]
    return [name, sha(entry), dsize, lib[0], lib[1], pool.put(lib[2]), ref]


def unpack(meta):
    """the record as dicts: name, entry_sha, dsize, code, len, sha, reference
    ("hang" or per cache dict(bytes, sha, last, error))"""
    st = meta["strings"]
    out = []
    for name, esha, dsize, code, n, h, ref in meta["cases"]:
        if ref != "hang":
            ref = [{"bytes": a, "sha": st[b], "last": c, "error": st[d]} for a, b, c, d in ref]
        out.append({"name": name, "entry_sha": esha, "dsize": dsize, "code": code, "len": n, "sha": st[h],
                    "reference": ref})
    return out


def main():
    from oracle.oracle import RefZseek
    z = load_zstd()
    assert z is not None, "libzstd 1.4.9 missing"
    ref = RefZseek()
    assert ref.versions["zstd"] == 10409, ref.versions
    pool = Pool()
    cases = []
    for name, entry, dsize, _, _ in zstd_craft.CASES:
        img, sizes = case_image(entry, dsize)
        cases.append(pack(pool, name, entry, dsize, libzstd_answer(z, entry, dsize),
                          ref_answers_guarded(ref, img, sum(sizes))))
    with open(os.path.join(OUT, "zstd_craft.json"), "w") as f:
        f.write('{"libzstd": 10409,\n "neighbour_entry_shas": %s,\n "strings": %s,\n "cases": [\n'
                % (json.dumps([sha(e) for e, _ in zstd_craft.NEIGHBOURS]), json.dumps(pool.strings, indent=0)))
        f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in cases))
        f.write("\n]}\n")
    print(len(cases), "cases;", sum(c[3] == 0 for c in cases), "decoded by libzstd;",
          sum(c[6] == "hang" for c in cases), "hang the reference reader")


if __name__ == "__main__":
    main()
