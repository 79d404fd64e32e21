#!/usr/bin/env python3
"""Wall time of the post commands with the rows uploaded per stage (the default) and once per command (`resident=True`), on the
README's post workload (run on the GPU box): 10 s x 1024 channels of 8-bit rows with one dispersed burst and one dead channel,

* `post.candidates_fil` over 64 DMs with `rfi=True` (flag, search, group, cut 256 x 256 planes), and
* `post.rfifind_fil(write_clean=True)` on a four-product file of the same length (1.28 GB of rows),

each configuration in FRESH processes (`--runs`, default 7: median and spread of the first call of a process) and, in every one of
those processes, `--repeat` further calls (default 3: the warm numbers; an earlier RFI timing differed between a fresh process and a
warm one, so both are recorded).  The resident runs also record the per-stage wall and device times of the library's result view.
`--parent ROOT`: a checkout of the parent commit with its library built -- the non-resident configurations are measured a second
time with ITS package and library, which shows whether the default path moved.  Prints one JSON object and, with `--out FILE`,
writes it there (profiles/candidates_resident.json).

    python tools/candidates_timing.py --out profiles/candidates_resident.json [--parent /path/to/parent/checkout]
"""
import argparse
import json
import os
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = dict(nchans=1024, nbits=8, fch1=1416.0 - 0.015625, foff=-0.03125, tsamp=32e-6, tstart=59000.0)
DM1, DM2, BURST_DM, BURST_ROW, DEAD_CHANNEL = 300.0, 363.0, 330.0, 150000, 17


def sigproc_header(nifs):
    def s(text):
        return struct.pack("<i", len(text)) + text.encode()
    out = s("HEADER_START") + s("source_name") + s("J0000+00")
    for key, val in (("machine_id", 0), ("telescope_id", 0), ("data_type", 1), ("nchans", HDR["nchans"]), ("nbits", HDR["nbits"]), ("nifs", nifs)):
        out += s(key) + struct.pack("<i", val)
    for key in ("fch1", "foff", "tsamp", "tstart"):
        out += s(key) + struct.pack("<d", HDR[key])
    return out + s("HEADER_END")


def make_files(directory, seconds):
    import numpy as np
    nrows, nchan = int(round(seconds / HDR["tsamp"])), HDR["nchans"]
    rng = np.random.default_rng(3)
    x = rng.integers(100, 156, size=(nrows, nchan), dtype=np.uint8)
    f = HDR["fch1"] + HDR["foff"] * np.arange(nchan)
    dly = (BURST_DM / 2.41e-4 * (f ** -2 - f[0] ** -2) / HDR["tsamp"] + 0.5).astype(np.int64)
    row = min(BURST_ROW, nrows // 2)
    for c in range(nchan):
        x[row + dly[c]: row + dly[c] + 5, c] += 12
    x[:, DEAD_CHANNEL] = 100
    one, four = os.path.join(directory, "burst.fil"), os.path.join(directory, "four.fil")
    with open(one, "wb") as fh:
        fh.write(sigproc_header(1) + x.tobytes())
    y = np.empty((nrows, 4, nchan), np.uint8)
    for p in range(4):
        y[:, p, :] = x if p == 0 else rng.integers(60 + 10 * p, 100 + 10 * p, size=(nrows, nchan), dtype=np.uint8)
    with open(four, "wb") as fh:
        fh.write(sigproc_header(4) + y.tobytes())
    return one, four, nrows


def worker(a):
    """one process: the command 1 + repeat times on a private copy of the file's directory entry (outputs land next to it)"""
    sys.path.insert(0, a.root)
    from frb_baseband_amd import post
    resident = dict(resident=True) if a.resident else {}
    calls = []
    for _ in range(1 + a.repeat):
        info = {}
        t0 = time.perf_counter()
        if a.command == "candidates":
            files, groups = post.candidates_fil(a.fil, DM1, dm2=DM2, dmstep=1.0, threshold=8.0, rfi=True, info=info, **resident)
            n = int(groups.size)
        else:
            files, _res = post.rfifind_fil(a.fil, write_clean=True, info=info, **resident)
            n = len(files)
        wall = time.perf_counter() - t0
        calls.append(dict(wall_ms=round(1e3 * wall, 3), n=n, row_uploads=info.get("row_uploads"),
                          stage_wall_ms=info.get("wall_ms"), stage_device_ms=info.get("device_ms")))
    print("RESULT " + json.dumps(calls))


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), each=[round(x, 3) for x in v])


def measure(a, command, fil, resident, root, lib):
    first, warm, stages = [], [], []
    env = dict(os.environ)
    if lib:
        env["FRBCH_LIB"] = lib
    n = None
    for _ in range(a.runs):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", command, "--fil", fil, "--root", root, "--repeat", str(a.repeat)]
        out = subprocess.run(cmd + (["--resident"] if resident else []), env=env, check=True, capture_output=True, text=True, timeout=a.limit).stdout
        calls = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
        first.append(calls[0]["wall_ms"])
        warm += [c["wall_ms"] for c in calls[1:]]
        stages.append(calls[0])
        n = calls[0]["n"]
        print(command, "resident" if resident else "default", root, [c["wall_ms"] for c in calls], file=sys.stderr, flush=True)
    res = dict(fresh_process_first_call_ms=spread(first), outputs=n, row_uploads=stages[0]["row_uploads"])
    if warm:
        res["same_process_repeated_calls_ms"] = spread(warm)
    if stages[0]["stage_wall_ms"]:
        for key in ("stage_wall_ms", "stage_device_ms"):
            res[key + "_median_of_first_calls"] = {k: round(statistics.median(s[key][k] for s in stages), 3) for k in stages[0][key]}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=7, help="fresh processes per configuration")
    ap.add_argument("--repeat", type=int, default=3, help="further calls inside every process")
    ap.add_argument("--seconds", type=float, default=10.0, help="length of the files")
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a process may take")
    ap.add_argument("--parent", default=None, help="checkout of the parent commit, library built")
    ap.add_argument("--commands", default="candidates,rfifind")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--fil", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    ap.add_argument("--resident", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        a.command = a.worker
        return worker(a)
    work = tempfile.mkdtemp(prefix="candidates_timing_")
    try:
        one, four, nrows = make_files(work, a.seconds)
        out = dict(workload=dict(rows=nrows, nchan=HDR["nchans"], nbits=8, seconds=a.seconds, dms=64, rfi=True, nt=256, ndm=256,
                                 row_image_bytes=nrows * HDR["nchans"], four_product_bytes=4 * nrows * HDR["nchans"]),
                   runs=a.runs, repeat=a.repeat)
        own = os.path.dirname(HERE)
        for command, fil in (("candidates", one), ("rfifind", four)):
            if command not in a.commands.split(","):
                continue
            r = out[command] = {}
            r["default"] = measure(a, command, fil, False, own, None)
            r["resident"] = measure(a, command, fil, True, own, None)
            if a.parent:
                r["default_parent_build"] = measure(a, command, fil, False, a.parent, os.path.join(a.parent, "frb_baseband_amd", "csrc", "libfrbch.so"))
            d, s = r["default"]["fresh_process_first_call_ms"]["median"], r["resident"]["fresh_process_first_call_ms"]["median"]
            r["resident_minus_default_ms"] = round(s - d, 3)
            print(command, json.dumps(r), file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
