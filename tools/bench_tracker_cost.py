"""What the tracker costs per step: the graph-replayed step of a PureMPC_Agent evaluation (evaluate.evaluate_agent, one episode
per environment) with a perception model (corner buildings, 5 % dropout, bounded noise), with tracker=dict(coast=...) against
tracker=None, alternating, --runs of each in one process.  The yardstick is the run without the tracker in the same process.
Prints the time per step of every run (host clock around the stepping loop, which ends in a synchronise, over the steps taken),
both ranges, the difference of the medians, and the tracker's totals.  The two kinds of run do not see the same episodes
(the agent acts on other rows), so the steps taken differ a little; the time is per step.

  python tools/bench_tracker_cost.py --envs 256 --runs 5
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--coast", type=int, default=10)
    ap.add_argument("--traffic", default="idm", choices=("constant", "idm"))
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from mpc_rl_for_avs_amd import evaluate, rollout
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent

    class Env:
        config = {"simulation_frequency": 30, "policy_frequency": 10, "observation": {"vehicles_count": 10}}

    dev = torch.device("cuda", 0)
    agent = PureMPC_Agent(Env(), dict(horizon=20, render=False, weight_speed=1, weight_control=1, weight_input_diff=1),
                          collision_cost=False)
    perception = dict(occlusion=True, occluders=evaluate.corner_buildings(), p_drop=0.05, sigma_pos=0.2, sigma_vel=0.3,
                      sigma_head=0.02, seed=args.seed)
    tracker = dict(coast=args.coast, alpha_pos=0.5, alpha_vel=0.5)

    def run(with_tracker):
        env = rollout.SyntheticIntersectionEnv(args.envs, device=dev, seed=args.seed, n_others=4, traffic=args.traffic)
        res = evaluate.evaluate_agent(agent, env, 1, seed=args.seed, use_graph=True, perception=dict(perception),
                                      tracker=dict(tracker) if with_tracker else None)
        return res.seconds / res.steps * 1e6, res

    run(False), run(True)                                    # warm-up: allocations, lazy initialisation
    us = {False: [], True: []}
    for i in range(args.runs):
        for with_tracker in (False, True):
            t, res = run(with_tracker)
            us[with_tracker].append(t)
            print(f"run {i} tracker={'on ' if with_tracker else 'off'} {t:8.1f} us/step  ({res.steps} steps, {args.envs} "
                  "environments)", flush=True)
    median = {}
    for with_tracker in (False, True):
        v = sorted(us[with_tracker])
        median[with_tracker] = v[len(v) // 2]
        print(f"tracker={'on ' if with_tracker else 'off'} min {v[0]:.1f}  median {v[len(v) // 2]:.1f}  max {v[-1]:.1f} us/step")
    print(f"difference of the medians {median[True] - median[False]:+.1f} us/step")
    print(f"tracker totals {res.tracker}; coasted_frac {res.summary()['coasted_frac']:.4f}")


if __name__ == "__main__":
    main()
