"""Worker of tests/test_gpu_host_calls.py (the library's switches are read once per process, so every leg is a run of this script).

usage: host_calls_worker.py fuzz <leg> <first index> <count> [<directory for the final states>]
           the sequences tests/host_calls.py draws for the leg's seeds, on the engine: one line per seed with a SHA-256 of every
           comparison point and the scalars, then -- behind "  # " -- what ran: launches, iterations, pairs, cold starts, stamps, replays
       host_calls_worker.py scenario <name> <out.npz>
           one of the four hand-written regressions (SCENARIOS): the state and the scalars after every batch, pairs per batch, counters
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd"), os.path.dirname(os.path.abspath(__file__))]
import hipims_mi as hp  # noqa: E402
from hipims_mi import synthetic as syn  # noqa: E402
import host_calls as hc  # noqa: E402

logs = []
hp.set_log_sink(lambda level, text: logs.append(text))
replays = lambda: sum("re-run with the plain divisions" in l for l in logs)

RAIN = np.array([[0.0, 600.0], [0.7, 200.0], [1.4, 50.0], [2.1, 0.0]])
STRONGER_RAIN = np.array([[0.0, 5000.0], [0.7, 3000.0], [1.4, 0.0], [2.1, 0.0]])


def scenario(name, out):
    states, scalars, pairs = [], [], []

    def batch(dom, n):
        before = dom.pair_stats()["pairs"]
        dom.step_batch(n)
        pairs.append(dom.pair_stats()["pairs"] - before)
        sc = dom.read_scalars()
        states.append(dom.download()); scalars.append([sc["time"], sc["timestep"]])

    if name in ("split_behind_boundary_pairs", "boundary_change_in_checkpoint"):
        st, bed, man = syn.s_rough(64, 37, manning=None, seed=31)
        dom = hp.Domain(64, 37, math_mode=hp.MATH_FAST)
        dom.upload(st, bed, man)
        dom.add_uniform(hp.UNIFORM_RAIN_INTENSITY, RAIN, 0.7, 2.1)
        dom.set_target_time(1e9)
        batch(dom, 8)
        if name == "split_behind_boundary_pairs":
            for _ in range(2):
                dom.step_begin(); dom.step_end()
        else:
            dom.state_save()
            dom.add_uniform(hp.UNIFORM_RAIN_INTENSITY, STRONGER_RAIN, 0.7, 2.1)
            dom.state_restore()
        batch(dom, 8)
    elif name == "replay_behind_pairs":
        st, bed, man = hc.rough_with_nulls(65, 37)
        dom = hp.Domain(65, 37, math_mode=hp.MATH_STRICT)
        dom.upload(st, bed, man)
        dom.set_target_time(1e9)
        for n in (6, 9, 5, 12):
            batch(dom, n)
    elif name in ("blockwise_load", "blockwise_load_open_edge"):
        st, bed, man = syn.s_dam(130, 64)
        dom = hp.Domain(130, 64, math_mode=hp.MATH_FAST)
        dom.upload(bed=bed, manning=man)
        if name == "blockwise_load":                           # the state arrives through upload_rows alone
            for y in range(0, 64, 16):
                dom.upload_rows(st[y:y + 16], y)
        else:                                                  # after a run, the grid comes back by rows with water standing on its edge ring
            dom.upload(st)
            dom.set_target_time(1e9)
            batch(dom, 6)
            cur = dom.download()
            for sl in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
                cur[sl] = (2.0, 2.0, 0.1, -0.1)
            for y in range(0, 64, 16):
                dom.upload_rows(cur[y:y + 16], y)
        dom.set_target_time(1e9)
        batch(dom, 20)
    else:
        raise SystemExit(f"unknown scenario {name}")
    counts, ps, sc = dom.launch_counts(), dom.pair_stats(), dom.read_scalars()
    np.savez(out, states=np.stack(states), scalars=np.array(scalars), pairs=np.array(pairs), launches=counts[0], iterations=sc["iterations"],
             cold_starts=ps["cold_starts"], stamped_ever=ps["stamped_ever"], replays=replays())
    dom.close()
    print(f"scenario {name}: pairs per batch {pairs} launches {counts[0]} iterations {sc['iterations']} cold starts {ps['cold_starts']} replays {replays()}")


SCENARIOS = ("split_behind_boundary_pairs", "boundary_change_in_checkpoint", "replay_behind_pairs", "blockwise_load", "blockwise_load_open_edge")


def fuzz(leg, first, count, outdir):
    for index in range(first, first + count):
        seed = hc.SEED_BASE[leg] + index
        seq = hc.make_sequence(seed, leg)
        before = replays()
        sim = hc.EngineSim(seq["cfg"])
        res = hc.execute(seq, sim)
        counts, ps, its = sim.dom.launch_counts(), sim.dom.pair_stats(), sim.dom.read_scalars()["iterations"]
        sim.close()
        if outdir:
            np.save(os.path.join(outdir, f"{leg}_{index}.npy"), res["points"][-1])
        print(f"seed {seed} {hc.digest(res) if res['finite'] else 'non-finite-state-not-compared'}  # launches {counts[0]} iterations {its} "
              f"pairs {ps['pairs']} cold_starts {ps['cold_starts']} stamped {ps['stamped_ever']} replays {replays() - before}", flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "scenario":
        scenario(sys.argv[2], sys.argv[3])
    else:
        fuzz(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] if len(sys.argv) > 5 else None)
