"""Generate tests/golden/lz4_linked_craft.json: what liblz4 1.9.3 and the
compiled reference reader make of every hand-built linked frame of
tests/lz4_linked_craft.py's CASES.

Run in the build container (needs /opt/conda's liblz4 1.9.3 and oracle/_ref
built by `make -C oracle ref`):

    python tests/golden/make_lz4_linked_craft.py

The record is make_lz4_craft.py's, made with its functions: per case liblz4's
verdict on the frame alone (LZ4F_decompress into a buffer of the declared size
+ LZ4F_SLACK bytes) and the reference reader's answers, cache 0 and 1, on a
seekable file that holds the frame between lz4_craft.NEIGHBOURS.  The table has
some 500 frames, so hashes are cut to their first 16 hex digits (H) and a case
takes one line.  Only data is written (names, numbers, hashes, strings);
"frame_sha" pins the frames, which are regenerated from the table.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lz4_craft  # noqa: E402
import lz4_linked_craft  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
LZ4F_SLACK = 1 << 16
H = 16

_spec = importlib.util.spec_from_file_location("make_lz4_craft", os.path.join(OUT, "make_lz4_craft.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
load_lz4, case_image = base.load_lz4, base.case_image


def sha(b) -> str:
    return base.sha(b)[:H]


def lz4f_verdict(lz, frame: bytes, dsize: int):
    err, got = base.lz4f_decode(lz, frame, dsize + LZ4F_SLACK)
    return {"ok": err == "", "error": err, "len": len(got), "sha": sha(got) if err == "" else ""}


def ref_answers(ref, img: bytes, total: int):
    out = base.ref_answers(ref, img, total)
    for a in out.values():
        a["sha"] = a["sha"][:H]
    return out


def main():
    from oracle.oracle import RefZseek
    lz = load_lz4()
    assert lz is not None and lz.LZ4_versionNumber() == 10903, "liblz4 1.9.3 missing"
    ref = RefZseek()
    assert ref.versions["lz4"] == 10903, ref.versions
    cases = []
    for name, frame, dsize, _ in lz4_linked_craft.CASES:
        img, total = case_image(frame, dsize)
        ans = base.ref_answers_guarded(ref, img, total)
        if ans != "hang":
            for a in ans.values():
                a["sha"] = a["sha"][:H]
        cases.append({"name": name, "frame_sha": sha(frame), "dsize": dsize, "lz4f": lz4f_verdict(lz, frame, dsize),
                      "reference": ans})
    with open(os.path.join(OUT, "lz4_linked_craft.json"), "w") as f:
        f.write('{"lz4f_slack": %d, "sha_digits": %d, "neighbour_frame_shas": %s,\n"cases": [\n' %
                (LZ4F_SLACK, H, json.dumps([sha(f) for f, _ in lz4_craft.NEIGHBOURS])))
        f.write(",\n".join(json.dumps(c) for c in cases))
        f.write("\n]}\n")
    print(len(cases), "cases;", sum(c["lz4f"]["ok"] for c in cases), "accepted by LZ4F_decompress alone;",
          sum(c["reference"] == "hang" for c in cases), "hang the reference reader")


if __name__ == "__main__":
    main()
