"""Worker of tests/test_gpu_host_calls_actors.py (the library's switches are read once per process, so every leg is a run of this script).

usage: host_calls_actors_worker.py fuzz <leg> <first index> <count> [<directory for the final states>]
           the sequences tests/host_calls_actors.py draws for the leg's seeds, on the engine: one line per seed with a SHA-256 of
           state, bed and links' records at every comparison point, the scalars and the checkpoint warnings, then -- behind "  # " --
           what ran: launches, iterations, pairs, replays, bed applies and the cells they changed, the links' `active` sum, and the
           pairs counted by batches that ran with a link group attached
       host_calls_actors_worker.py scenario <name> <out.npz>
           one of the two hand-written scenarios (host_calls_actors.SCENARIOS)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hipims-ocl_amd"), os.path.dirname(os.path.abspath(__file__))]
import hipims_mi as hp  # noqa: E402
import host_calls_actors as ha  # noqa: E402

logs = []
hp.set_log_sink(lambda level, text: logs.append(text))
replays = lambda: sum("re-run with the plain divisions" in l for l in logs)
restore_warnings = lambda: sum("hp_state_restore:" in l for l in logs)


def scenario(name, out):
    sim = ha.ActorEngineSim(ha.scenario_cfg(name), warnings=restore_warnings)
    res = ha.run_scenario(name, sim)
    info = sim.dom.bed_info()
    np.savez(out, states=np.stack(res["states"]), beds=np.stack(res["beds"]), scalars=np.array(res["scalars"]),
             records=np.concatenate([r.view(np.uint8) for r in res["records"]]) if res["records"] else np.zeros(0, np.uint8),
             pairs=np.array(sim.pairs_by_batch), replays=replays(), warnings=res["warnings"], applies=info["applies"], changed_total=info["changed_total"])
    sim.close()
    print(f"scenario {name}: pairs per batch {sim.pairs_by_batch} replays {replays()} applies {info['applies']} changed {info['changed_total']}")


def fuzz(leg, first, count, outdir):
    for index in range(first, first + count):
        seed = ha.SEED_BASE[leg] + index
        seq = ha.make_actor_sequence(seed, leg)
        before = replays()
        sim = ha.ActorEngineSim(seq["cfg"], warnings=restore_warnings)
        res = ha.execute(seq, sim)
        counts, ps, its, bed = sim.dom.launch_counts(), sim.dom.pair_stats(), sim.dom.read_scalars()["iterations"], sim.bed_totals()
        active = max([sim.links_active] + [int(r["active"].sum()) for r in res["reads"]])
        sim.close()
        if outdir:
            np.save(os.path.join(outdir, f"{leg}_{index}.npy"), res["points"][-1][0])
        print(f"seed {seed} {ha.digest(res) if res['finite'] else 'non-finite-state-not-compared'}  # launches {counts[0]} iterations {its} "
              f"pairs {ps['pairs']} replays {replays() - before} applies {bed[0]} changed {bed[1]} links_active {active} "
              f"pairs_with_links {sim.pairs_with_links}", flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "scenario":
        scenario(sys.argv[2], sys.argv[3])
    else:
        fuzz(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] if len(sys.argv) > 5 else None)
