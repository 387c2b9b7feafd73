"""HBM bytes the launches of ONE ngp_factor_predict_long call move, from rocprofv3 counters, beside
the algorithmic bytes the library books for them.

    rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d FETCH_DIR -- \
        python scripts/long_horizon_pmc.py run
    rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d WRITE_DIR -- \
        python scripts/long_horizon_pmc.py run
    python scripts/long_horizon_pmc.py parse FETCH_DIR WRITE_DIR OUT.json

(one counter pass per run).  `run` copies 1 GiB with the library's stream_copy_kernel first — the
units of the two counters are calibrated on that launch, as scripts/pmc_to_json.py does — then makes
REPS variances-only queries at P = 64, n = 2,047, m = 365."""
import collections
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, N, M, REPS = 64, 2047, 365, 3


def run():
    import numpy as np
    import __graft_entry__ as ge
    ge.build()
    from nowcastautogp_amd import _lib
    from nowcastautogp_amd.synthetic import make_workload
    ctx = _lib.Context(0)
    ctx.microbench_hbm(1 << 30)
    w = make_workload("C1", n=N, P=P, D=1, d=1, m=4)
    t_new = w.t[-1] + (w.t[1] - w.t[0]) * np.arange(1, M + 1)
    f = ctx.factor(w.programs, w.t, w.y)
    for _ in range(REPS):
        mu, var, _, info = f.predict_long(t_new, want_sigma=False)
        assert not info.any()
    f.close()
    ctx.close()


def load(d, counter):
    files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    agg, cnt = collections.defaultdict(float), collections.Counter()
    for row in csv.DictReader(open(files[0])):
        if row["Counter_Name"] != counter:
            continue
        name = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("ngp::", "").strip()
        agg[name] += float(row["Counter_Value"])
        cnt[name] += 1
    return agg, cnt


def parse(fetch_dir, write_dir, out):
    fetch, nf = load(fetch_dir, "FETCH_SIZE")
    write, nw = load(write_dir, "WRITE_SIZE")
    gib = float(1 << 30)
    cal_r = gib / (fetch["stream_copy_kernel"] / nf["stream_copy_kernel"])
    cal_w = gib / (write["stream_copy_kernel"] / nw["stream_copy_kernel"])
    n0, q1 = N // 64 * 64, 1 + N % 64 + M
    qpad = (q1 + 63) // 64 * 64
    # the solve: L once per 256-column workgroup tile, the panel once in and once out — the count
    # of a panel that stays on chip — and what the left-looking sweep adds to it: block column j of
    # the solved panel is read back by every later step (what the library books is their sum)
    once = 8.0 * P * ((qpad + 255) // 256 * n0 * n0 / 2 + 2.0 * qpad * n0)
    reread = 8.0 * P * qpad * n0 * (n0 // 64 - 1) / 2.0
    algorithmic = {"long_solve_kernel": once + reread, "long_fill_kernel": 8.0 * P * qpad * n0}
    res_extra = {"solve_bytes_panel_once": once, "solve_bytes_panel_read_back": reread}
    res = {"shape": dict(P=P, n=N, m=M, want_sigma=False),
           "calibration": {"bytes_per_FETCH_SIZE_unit": cal_r, "bytes_per_WRITE_SIZE_unit": cal_w},
           **res_extra, "kernels": {}}
    for k in sorted(fetch):
        if not k.startswith("long_"):
            continue
        r = fetch[k] * cal_r / nf[k]
        wr = write.get(k, 0.0) * cal_w / max(nw.get(k, 1), 1)
        res["kernels"][k] = {"launches": nf[k], "read_bytes_per_launch": r, "written_bytes_per_launch": wr,
                             "moved_bytes_per_launch": r + wr, "algorithmic_bytes_per_launch": algorithmic.get(k)}
        print(k, json.dumps(res["kernels"][k]))
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        parse(*sys.argv[2:5])
