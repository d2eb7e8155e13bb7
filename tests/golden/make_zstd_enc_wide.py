"""Records tests/golden/zstd_enc_wide.json: size and SHA-256 of the frames that
the wide entry of the zstd compressor's CPU shim (zenc_wide_compress of
tests/native/zstd_enc_wide_shim.cpp over libzseek_amd/csrc/zstd_enc_wide_dev.h)
writes for the inputs at the search's edges (tests/zstd_wide_util.py).  Run
once the decodes of tests/test_zstd_enc_wide.py pass, at the commit whose wide
bytes are the record, and never again unless the wide format is changed on
purpose:

    python tests/golden/make_zstd_enc_wide.py

tests/test_zstd_enc_wide.py recomputes the hashes with the same shim.
"""
from __future__ import annotations

import hashlib
import json
import pathlib
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parents[2]
OUT = pathlib.Path(__file__).with_name("zstd_enc_wide.json")
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import zstd_wide_util as wu  # noqa: E402


def inputs(oracle):
    return wu.edge_inputs(oracle) + [("cross_" + k, v, 0) for k, v in sorted(wu.cross_block_inputs().items())]


def hashes(L, oracle) -> dict:
    rec = {}
    for name, content, ck in inputs(oracle):
        frame = wu.compress(L, content, ck)
        rec[name] = {"input_sha256": hashlib.sha256(content.tobytes()).hexdigest(), "checksum": int(ck),
                     "size": len(frame), "sha256": hashlib.sha256(frame).hexdigest()}
    return rec


if __name__ == "__main__":
    from oracle.oracle import Oracle
    with tempfile.TemporaryDirectory() as d:
        rec = hashes(wu.load_shim(d), Oracle())
    OUT.write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT, len(rec), "entries")
