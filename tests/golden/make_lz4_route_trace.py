"""tests/golden/lz4_route_trace.json from kernel traces of scripts/lz4_route_probe.py.

    python tests/golden/make_lz4_route_trace.py RUN_DIR [--full OUT.json]

RUN_DIR/<setting>/ holds one probe run per switch setting of the probe's
SETTINGS, each made on an MI355X with

    ZSEEK_...=... rocprofv3 --kernel-trace --output-format csv -d RUN_DIR/<setting> -- \
        python scripts/lz4_route_probe.py RUN_DIR/<setting>/probe.json

The committed file was recorded from the library as it was before the launch
sequence moved into csrc/lz4_route.h: it is the reference the plan is held to
(tests/test_lz4_route.py), so re-record it only from a library whose routing
is meant to be the new truth.

Per setting and case: the requests the probe wrote down and the ordered kernel
base names (the text before any `<` or `(`) between two separator launches,
without the kernels of PLUMBING -- the reader's transfers, descriptors and
gathers and the runtime's own fills and copies, which no LZ4 routing decides.
--full: the same cut with full kernel names and grid / workgroup sizes, for
comparing two libraries."""
from __future__ import annotations

import csv
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "scripts"))
import lz4_route_probe as probe  # noqa: E402

PLUMBING = {"h2d_small_kernel", "d2h_small_kernel", "d2h_flag_kernel", "image_desc_kernel", "range_scan_kernel",
            "range_gather_kernel", "range_result_kernel", "plan_touch_kernel", "plan_compact_kernel",
            "plan_segments_kernel", "plan_fix_kernel"}


def base(name: str) -> str:
    """`void zsk::(anonymous namespace)::k<3, true>(args) [clone .kd]` -> `k`"""
    name = re.sub(r"\(anonymous namespace\)::", "", name.strip())
    name = re.split(r"[<(]", name, maxsplit=1)[0].strip()
    return name.split(" ")[-1].split("::")[-1].removesuffix(".kd")


def dispatches(run_dir: str):
    files = glob.glob(os.path.join(run_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (run_dir, files)
    rows = list(csv.DictReader(open(files[0])))
    # launch order (a read of two batches runs them on two streams: their start times interleave)
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    shape = [c for c in (rows[0] if rows else {}) if c.startswith(("Grid_Size", "Workgroup_Size"))]
    return [(r["Kernel_Name"], [int(r[c]) for c in shape]) for r in rows]


def cut(run_dir: str):
    """-> (probe.json, per case the [(full name, shape)] it launched)"""
    meta = json.load(open(os.path.join(run_dir, "probe.json")))
    groups, seen = [], 0
    for name, shape in dispatches(run_dir):
        b = base(name)
        if b == meta["separator"]:
            seen += 1
            groups.append([])
        elif seen and b not in PLUMBING and not b.startswith("__amd_rocclr_"):
            groups[-1].append((name, shape))
    assert seen == len(meta["cases"]) + 1, (run_dir, seen, len(meta["cases"]))
    assert not groups[-1], groups[-1]
    return meta, groups[:-1]


def main(argv) -> None:
    run = argv[1]
    out, full = {}, {}
    for setting, env in probe.SETTINGS.items():
        meta, groups = cut(os.path.join(run, setting))
        assert meta["env"] == env, (setting, meta["env"])
        out[setting] = {"env": env, "names": meta["names"],
                        "cases": {c["name"]: {"requests": c["requests"], "kernels": [base(k) for k, _ in g]}
                                  for c, g in zip(meta["cases"], groups)}}
        full[setting] = {c["name"]: [[k, s] for k, s in g] for c, g in zip(meta["cases"], groups)}
    if "--full" in argv:
        json.dump(full, open(argv[argv.index("--full") + 1], "w"), indent=0)
    else:
        with open(os.path.join(HERE, "lz4_route_trace.json"), "w") as f:
            json.dump({"separator": probe.SEPARATOR, "settings": out}, f, separators=(",", ":"))
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv)
