"""Generate tests/golden/exec_craft.json: what liblz4 1.9.3, libzstd 1.4.9 and
the compiled reference reader make of every hand-built frame of
tests/exec_craft.py (its LZ4 table, then its zstd forms under "z:" names).

Run in the build container (needs /opt/conda's liblz4 1.9.3 and libzstd 1.4.9
and oracle/_ref built by `make -C oracle ref`):

    python tests/golden/make_exec_craft.py

The record is make_lz4_linked_craft.py's, made with make_lz4_craft.py's and
make_zstd_craft.py's functions: per case the library's verdict on the frame
alone (decoded or not, the length, the hash) and the reference reader's
answers, cache 0 and 1, on a seekable file that holds the frame between the
format's two intact neighbours (lz4_craft.NEIGHBOURS, zstd_craft.NEIGHBOURS).
Hashes are cut to their first 16 hex digits (H) and a case takes one line.
Only data is written (names, numbers, hashes, strings); "frame_sha" pins the
frames, which are regenerated from the table.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import exec_craft  # noqa: E402
import lz4_craft  # noqa: E402
import zstd_craft  # noqa: E402
import zstd_util  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
LZ4F_SLACK = 1 << 16
H = 16


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(OUT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


base = _load("make_lz4_craft")
zbase = _load("make_zstd_craft")


def sha(b) -> str:
    return base.sha(b)[:H]


def all_cases(with_fmt: bool = False):
    """(name, frame, dsize, expected bytes) of the LZ4 table, then of the zstd
    forms as "z:" + name"""
    for name, f, ds, want in exec_craft.CASES:
        yield ("lz4", name, f, ds, want) if with_fmt else (name, f, ds, want)
    for name, f, ds, want in exec_craft.ZCASES:
        yield ("zstd", "z:" + name, f, ds, want) if with_fmt else ("z:" + name, f, ds, want)


def neighbours(fmt: str):
    """the decoded bytes of the neighbour before and after a case"""
    nb = lz4_craft.NEIGHBOURS if fmt == "lz4" else zstd_craft.NEIGHBOURS
    return nb[0][1], nb[1][1]


def case_image(fmt: str, frame: bytes, dsize: int):
    if fmt == "lz4":
        return base.case_image(frame, dsize)
    img, sizes = zbase.case_image(frame, dsize)
    return img, sum(sizes)


def ref_answers(ref, img: bytes, total: int):
    out = base.ref_answers(ref, img, total)
    for a in out.values():
        a["sha"] = a["sha"][:H]
    return out


def main():
    from oracle.oracle import RefZseek
    lz = base.load_lz4()
    assert lz is not None and lz.LZ4_versionNumber() == 10903, "liblz4 1.9.3 missing"
    z = zbase.load_zstd()
    assert z is not None, "libzstd 1.4.9 missing"
    ref = RefZseek()
    assert ref.versions["lz4"] == 10903 and ref.versions["zstd"] == 10409, ref.versions
    cases = []
    for fmt, name, frame, dsize, _ in all_cases(with_fmt=True):
        if fmt == "lz4":
            err, got = base.lz4f_decode(lz, frame, dsize + LZ4F_SLACK)
            lib = {"ok": err == "", "len": len(got), "sha": sha(got) if err == "" else ""}
        else:
            got, code = zstd_util.decode(z, frame, dsize)
            lib = {"ok": code == 0, "len": len(got), "sha": sha(got) if code == 0 else ""}
        img, total = case_image(fmt, frame, dsize)
        ans = base.ref_answers_guarded(ref, img, total)
        if ans != "hang":
            for a in ans.values():
                a["sha"] = a["sha"][:H]
        cases.append({"name": name, "frame_sha": sha(frame), "dsize": dsize, "lib": lib, "reference": ans})
    with open(os.path.join(OUT, "exec_craft.json"), "w") as f:
        f.write('{"lz4f_slack": %d, "sha_digits": %d, "neighbour_frame_shas": %s, "zstd_neighbour_shas": %s,\n"cases": [\n' %
                (LZ4F_SLACK, H, json.dumps([sha(f) for f, _ in lz4_craft.NEIGHBOURS]),
                 json.dumps([sha(f) for f, _ in zstd_craft.NEIGHBOURS])))
        f.write(",\n".join(json.dumps(c) for c in cases))
        f.write("\n]}\n")
    print(len(cases), "cases;", sum(c["lib"]["ok"] for c in cases), "decoded by the libraries alone;",
          sum(c["reference"] == "hang" for c in cases), "hang the reference reader")


if __name__ == "__main__":
    main()
