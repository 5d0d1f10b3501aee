"""The reference's model comparison (main/model_comparison.py) on the synthetic intersection: every agent evaluated in closed
loop on the same episodes (evaluate.compare), one JSON line per agent with model_comparison's five numbers (success and
collision rate in %, average steps, average speed, average travel time) and the throughput.  --metrics adds the safety and
comfort metrics of every agent's episodes (evaluate.DriveMetrics: near misses, time on a collision course, braking, jerk,
route keeping; a value that does not exist, such as the closest gap when no vehicle was met, prints as null).

Agents: pure MPC with the collision cost off and on, the iterative-linear (LTV) agent, and MPC-RL - an SB3 `.zip` given with
--mpcrl, or with --fixture the v0 PPO (gSDE) policy rebuilt from tests/golden/sb3_policies.npz.

  python tools/compare_models.py --envs 256 --episodes-per-env 1 --fixture
  python tools/compare_models.py --metrics --traffic idm --envs 256 --fixture
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--episodes-per-env", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--deterministic", action="store_true", help="MPC-RL acts with the policy's mean")
    ap.add_argument("--traffic", default="constant", choices=("constant", "idm"),
                    help="the other vehicles: constant velocity on the approach lanes, or IDM on turning routes")
    ap.add_argument("--metrics", action="store_true", help="also the safety and comfort metrics (evaluate.DriveMetrics)")
    src = ap.add_mutually_exclusive_group()
    src.add_argument("--mpcrl", help="an SB3 checkpoint (.zip) of the reference's MPC-RL agent")
    src.add_argument("--fixture", action="store_true", help="MPC-RL: the v0 PPO policy of tests/golden/sb3_policies.npz")
    args = ap.parse_args()

    import math

    import torch
    from mpc_rl_for_avs_amd import evaluate, rollout
    from mpc_rl_for_avs_amd.engine import MPCEngine
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
    from mpc_rl_for_avs_amd.pure_mpc_linear import IterativeLinearMPC_Agent

    class Env:          # what the agents read of the reference's highway-env configuration
        config = {"simulation_frequency": 30, "policy_frequency": 10, "observation": {"vehicles_count": 10}}

    cfg = dict(horizon=20, render=False, weight_speed=1, weight_control=1, weight_input_diff=1)
    dev = torch.device("cuda", 0)
    agents = {"pure_mpc": PureMPC_Agent(Env(), dict(cfg), collision_cost=False),
              "pure_mpc_collision": PureMPC_Agent(Env(), dict(cfg), collision_cost=True),
              "ltv": IterativeLinearMPC_Agent(Env(), dict(cfg))}
    path = args.mpcrl
    tmp = None
    if args.fixture:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import sde_host
        tmp = tempfile.TemporaryDirectory()
        path = sde_host.sb3_zip(tmp.name, "ppo_v0")
    if path:
        agents["mpcrl"], _ = rollout.MPCRLAgent.from_sb3(path, MPCEngine(horizon=20, device=0), device=dev)
    make_env = lambda: rollout.SyntheticIntersectionEnv(args.envs, device=dev, seed=args.seed, n_others=4,
                                                         traffic=args.traffic)
    for name, agent in agents.items():
        s = evaluate.compare({name: agent}, make_env, args.episodes_per_env, deterministic=args.deterministic,
                             seed=args.seed, metrics=args.metrics)[name]
        s = {k: (None if isinstance(v, float) and not math.isfinite(v) else v) for k, v in s.items()}
        print(json.dumps(dict(agent=name, traffic=args.traffic, envs=args.envs, episodes_per_env=args.episodes_per_env, **s)), flush=True)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
