"""What the sensing latency costs per step: the graph-replayed step of a PureMPC_Agent evaluation (evaluate.evaluate_agent, one
episode per environment) with a perception model (corner buildings, 5 % dropout, bounded noise) and an actuator model with a
steering lag of 0.2 s and the environment's limits (the step of tools/bench_compensation_cost.py), with latency=--steps - one
more launch per step, which keeps the scene and hands on an older one - against latency=None, --runs of each in one process,
in both orders (off then on in the even runs, on then off in the odd ones).  The yardstick is the run without the stage in the
same process.  --steps 0 (the default) is the identity: the same episodes, the cost of the launch and its copy alone.  With
--steps above 0 the agent acts on older scenes, so the two kinds of run see different episodes and the difference is what the
latency does to the whole step, not the price of its launch.  --compensate adds the matching compensator to the run with the
stage (mpc_compensate_stale above --steps 0).  Prints the time per step of every run (host clock around the stepping loop,
which ends in a synchronise, over the steps taken), both ranges, the difference of the medians, and the stage's totals.

  python tools/bench_latency_cost.py --envs 256 --runs 6
  python tools/bench_latency_cost.py --envs 256 --runs 6 --steps 2 --compensate
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
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=0, help="the sensing latency in policy steps (0..7)")
    ap.add_argument("--compensate", action="store_true", help="the run with the stage also gets the matching compensator")
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
    actuator = dict(delay=0, tau=(0.0, 0.2), limits="env")

    def run(with_stage):
        env = rollout.SyntheticIntersectionEnv(args.envs, device=dev, seed=args.seed, n_others=4, traffic=args.traffic)
        res = evaluate.evaluate_agent(agent, env, 1, seed=args.seed, use_graph=True, perception=dict(perception),
                                      actuation=dict(actuator), latency=args.steps if with_stage else None,
                                      compensation=True if with_stage and args.compensate else None)
        return res.seconds / res.steps * 1e6, res

    run(False), run(True)                                    # warm-up: allocations, lazy initialisation
    us, steps, totals = {False: [], True: []}, {False: set(), True: set()}, None
    for i in range(args.runs):
        for with_stage in ((False, True), (True, False))[i % 2]:
            t, res = run(with_stage)
            us[with_stage].append(t)
            steps[with_stage].add(res.steps)
            totals = (res.latency, res.compensation) if with_stage else totals
            print(f"run {i} latency={'on ' if with_stage else 'off'} {t:8.1f} us/step  ({res.steps} steps, {args.envs} "
                  "environments)", flush=True)
    median = {}
    for with_stage in (False, True):
        v = sorted(us[with_stage])
        median[with_stage] = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        print(f"latency={'on ' if with_stage else 'off'} min {v[0]:.1f}  median {median[with_stage]:.1f}  max {v[-1]:.1f} us/step")
    print(f"difference of the medians {median[True] - median[False]:+.1f} us/step (latency {args.steps} steps"
          f"{', compensated' if args.compensate else ''}); steps taken without the stage {sorted(steps[False])}, with it "
          f"{sorted(steps[True])}")
    print(f"latency totals {totals[0]}" + (f"; compensation totals {totals[1]}" if args.compensate else ""))


if __name__ == "__main__":
    main()
