"""What the episode trace recorder costs per step: the graph-replayed step of a PureMPC_Agent evaluation (evaluate.evaluate_agent,
one episode per environment) with trace=dict(keep="all", window=200) against trace=None, alternating, --runs of each in one
process.  Prints the time per step of every run (host clock around the stepping loop, which ends in a synchronise, over the
steps taken), both ranges, and the recorder's memory against the layout formula.

  python tools/bench_trace_cost.py --envs 256 --runs 5
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
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--traffic", default="constant", choices=("constant", "idm"))
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
    trace = dict(keep="all", window=args.window, capacity=args.envs)

    def run(with_trace):
        env = rollout.SyntheticIntersectionEnv(args.envs, device=dev, seed=args.seed, n_others=4, traffic=args.traffic)
        res = evaluate.evaluate_agent(agent, env, 1, seed=args.seed, use_graph=True, trace=dict(trace) if with_trace else None)
        return res.seconds / res.steps * 1e6, res

    run(False), run(True)                                    # warm-up: allocations, lazy initialisation
    us = {False: [], True: []}
    for i in range(args.runs):
        for with_trace in (False, True):
            t, res = run(with_trace)
            us[with_trace].append(t)
            print(f"run {i} trace={'on ' if with_trace else 'off'} {t:8.1f} us/step  ({res.steps} steps, {args.envs} environments)",
                  flush=True)
    for with_trace in (False, True):
        v = sorted(us[with_trace])
        print(f"trace={'on ' if with_trace else 'off'} min {v[0]:.1f}  median {v[len(v) // 2]:.1f}  max {v[-1]:.1f} us/step")
    tr = res.traces
    formula = evaluate.EpisodeTrace.bytes_for(args.envs, rollout.VEHICLES_COUNT, args.window, args.envs)
    print(f"kept {tr.counts['kept']} of {tr.counts['matched']} episodes; recorder memory {tr.nbytes} B "
          f"({tr.nbytes / 2 ** 20:.1f} MiB), layout formula {formula} B")
    for B, W, C in ((256, 200, 64), (8192, 50, 64)):
        n = evaluate.EpisodeTrace.bytes_for(B, rollout.VEHICLES_COUNT, W, C)
        print(f"layout formula: B={B} W={W} C={C} R={rollout.VEHICLES_COUNT}: {n} B ({n / 2 ** 20:.1f} MiB)")


if __name__ == "__main__":
    main()
