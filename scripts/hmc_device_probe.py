"""One HMC move through the host loop (autogp._hmc_move: a library call and a dozen numpy operations
per leapfrog) against the same move through ngp_grad_job_hmc (hmc_config["device"]: one call per
move), DESIGN.md section 4.23.  Same build, same box, same session; the two alternate.

  * per size: wall time of one move of 10 leapfrogs, median of REPS alternating pairs, and — in a
    separate pass with the profile switched on — the device time of the move's launches;
  * the vignette-scale fit of scripts/vignette_fit_probe.py with and without the key, alternating,
    FITS times each.
Usage: python scripts/hmc_device_probe.py [out.txt]   (REPS / FITS from the environment)"""
import datetime as dt
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge

ge.build()
from nowcastautogp_amd import autogp, nowcast as nc
from nowcastautogp_amd.synthetic import make_workload

REPS = int(os.environ.get("REPS", "15"))
FITS = int(os.environ.get("FITS", "3"))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def data_of(n, P):
    w = make_workload("C2", n=n, P=P, D=1)
    d0 = dt.date(2000, 1, 2)
    return nc.create_transformed_data([d0 + dt.timedelta(weeks=i) for i in range(n)], w.y, transformation=float)


eng = autogp.HipEngine(0)
say(f"one move of 10 leapfrogs, eps 0.02; median of {REPS} alternating pairs")
say(f"{'n':>5} {'items':>5} | {'host loop ms':>12} {'one call ms':>11} {'ratio':>6} | "
    f"{'device ms host':>14} {'device ms call':>14}")
for n, P in ((21, 24), (62, 24), (104, 24), (208, 24), (208, 64)):
    base = nc.make_and_fit_model(data_of(n, P), engine=eng, seed=3, n_particles=P, n_mcmc=1, n_hmc=1)
    snap = base.to_dict()
    t, y = base._obs()

    def move(device):
        m = autogp.GPModel.from_dict(snap, engine=eng)      # the same particles and draws every time
        t0 = time.perf_counter()
        autogp._hmc_move([m], t, [y], 10, 0.02, None, device)
        return (time.perf_counter() - t0) * 1e3

    for dev in (False, True):
        move(dev)                                            # warm
    wall = {False: [], True: []}
    for _ in range(REPS):
        for dev in (False, True):
            wall[dev].append(move(dev))
    devms = {}
    eng.ctx.profile_enable(True)
    for dev in (False, True):
        eng.ctx.profile_reset()
        move(dev)
        devms[dev] = sum(v["ms"] for v in eng.ctx.profile_get().values())
    eng.ctx.profile_enable(False)
    h, d = statistics.median(wall[False]), statistics.median(wall[True])
    say(f"{n:>5} {P:>5} | {h:>12.3f} {d:>11.3f} {h / d:>6.2f} | {devms[False]:>14.3f} {devms[True]:>14.3f}")

nv = 208
datav = data_of(nv, 24)
vs = dict(n_particles=24, smc_data_proportion=0.1, n_mcmc=50, n_hmc=20)
nc.make_and_fit_model(datav, engine=eng, seed=5, n_particles=24, smc_data_proportion=0.5, n_mcmc=2, n_hmc=2)
fit = {False: [], True: []}
for _ in range(FITS):
    for dev in (False, True):
        t0 = time.perf_counter()
        nc.make_and_fit_model(datav, engine=eng, seed=11, hmc_config={"device": dev}, **vs)
        fit[dev].append(time.perf_counter() - t0)
say(f"vignette-scale fit (n = {nv}, 24 particles, n_mcmc 50, n_hmc 20), alternating, {FITS} each:")
say("  host loop : " + "  ".join(f"{v:.2f}" for v in fit[False]) + f"  s   median {statistics.median(fit[False]):.2f}")
say("  one call  : " + "  ".join(f"{v:.2f}" for v in fit[True]) + f"  s   median {statistics.median(fit[True]):.2f}")
eng.ctx.close()
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
