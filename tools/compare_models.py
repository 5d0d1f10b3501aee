"""The reference's model comparison (main/model_comparison.py) on the synthetic intersection: every agent evaluated in closed
loop on the same episodes (evaluate.compare), one JSON line per agent with model_comparison's five numbers (success and
collision rate in %, average steps, average speed, average travel time) and the throughput.  --metrics adds the safety and
comfort metrics of every agent's episodes (evaluate.DriveMetrics: near misses, time on a collision course, braking, jerk,
route keeping; a value that does not exist, such as the closest gap when no vehicle was met, prints as null).
--range, --occlusion, --dropout and the three --sigma-* flags put a perception model between the environment and every agent
(evaluate.Perception: the agents act on what the ego sees, the numbers keep describing the true scene); the flags are echoed
in the JSON line, which then also holds the share of present rows that were seen, occluded, out of range and dropped.
--track-coast, --track-gate, --track-alpha-pos and --track-alpha-vel put a tracker behind the perception model (or the true
observation; evaluate.Tracker): a vehicle that vanishes for up to --track-coast steps stays in the observation at its last
velocity, measurements within --track-gate metres of a track are smoothed by the two gains.  Any of them switches it on; they
are echoed in the JSON line, which then also holds coasted_frac, the share of the agent's rows that were coasted.
--act-delay, --act-tau-*, --act-rate-*, --act-sigma-*, --act-p-hold, --act-steer-offset and --act-limits put an actuator model
between every agent and the environment (evaluate.Actuation: transport delay in policy steps, first-order lag, rate limit,
noise, lost commands, a steering offset, saturation); any of them switches it on; they are echoed in the JSON line, which then
also holds the act_* shares and mean deviations.  tools/robustness_sweep.py runs the comparison over a grid of them.
--compensate puts the delay compensator that matches that actuator model in front of every agent (evaluate.Compensation.matching:
the agents act on the scene predicted to the moment their command takes effect); the JSON line then also holds the
compensator's own prediction error, comp_pos_err_mean and comp_pos_err_max [m].
--sense-delay N hands every agent's pipeline (perception model, tracker, agent) the true scene of N policy steps ago
(evaluate.Latency); the JSON line then also holds sense_stale_mean and sense_ego_lag_mean / sense_ego_lag_max [m].  With
--compensate the compensator matches the actuator model and the sensing delay, whichever is given.

Agents: pure MPC with the collision cost off and on, the iterative-linear (LTV) agent, and MPC-RL - an SB3 `.zip` given with
--mpcrl, or with --fixture the v0 PPO (gSDE) policy rebuilt from tests/golden/sb3_policies.npz.  --ppo PATH adds the reference's
fourth model, the end-to-end PPO baseline (rollout.PPOAgent: the policy's outputs are the controls, no MPC), from a checkpoint
in the layout ActorCritic.save_sb3 writes; --ppo-random adds it with a seeded untrained policy, so the row exists anywhere.

  python tools/compare_models.py --envs 256 --episodes-per-env 1 --fixture
  python tools/compare_models.py --metrics --traffic idm --envs 256 --fixture
  python tools/compare_models.py --metrics --traffic idm --occlusion buildings --range 60 --sigma-pos 0.2
  python tools/compare_models.py --metrics --traffic idm --occlusion buildings --dropout 0.05 --track-coast 10
  python tools/compare_models.py --metrics --traffic idm --act-delay 2 --act-tau-steer 0.2 --act-limits env
  python tools/compare_models.py --metrics --traffic idm --act-delay 3 --act-limits env --compensate
  python tools/compare_models.py --metrics --traffic idm --sense-delay 2 --act-delay 1 --act-limits env --compensate
  python tools/compare_models.py --metrics --traffic idm --interaction --envs 256
  python tools/compare_models.py --envs 256 --fixture --ppo baseline.zip
  python tools/compare_models.py --traffic idm --trace failed --trace-window 50 --trace-dir out

--trace KEEP keeps the step-by-step record of the episodes that ended as KEEP says (evaluate.EpisodeTrace: the last
--trace-window steps of at most --trace-capacity episodes per model) and writes one --trace-dir/<model>.npz per model;
tools/show_episode.py prints an episode of such a file.  The JSON line then also names the file and the episodes matched,
kept and dropped.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class Env:          # what the agents read of the reference's highway-env configuration
    config = {"simulation_frequency": 30, "policy_frequency": 10, "observation": {"vehicles_count": 10}}


def build_agents(dev, seed=0, mpcrl=None, fixture=False, ppo=None, ppo_random=False):
    """-> ({name: agent}, a TemporaryDirectory to clean up or None): pure MPC without and with the collision cost, the
    iterative-linear agent, and where asked for MPC-RL and the end-to-end PPO baseline"""
    import torch
    from mpc_rl_for_avs_amd import rollout
    from mpc_rl_for_avs_amd.engine import MPCEngine
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent
    from mpc_rl_for_avs_amd.pure_mpc_linear import IterativeLinearMPC_Agent
    cfg = dict(horizon=20, render=False, weight_speed=1, weight_control=1, weight_input_diff=1)
    agents = {"pure_mpc": PureMPC_Agent(Env(), dict(cfg), collision_cost=False),
              "pure_mpc_collision": PureMPC_Agent(Env(), dict(cfg), collision_cost=True),
              "ltv": IterativeLinearMPC_Agent(Env(), dict(cfg))}
    path, tmp = mpcrl, None
    if fixture:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import sde_host
        tmp = tempfile.TemporaryDirectory()
        path = sde_host.sb3_zip(tmp.name, "ppo_v0")
    if path:
        agents["mpcrl"], _ = rollout.MPCRLAgent.from_sb3(path, MPCEngine(horizon=20, device=0), device=dev)
    if ppo:
        agents["ppo"], _ = rollout.PPOAgent.from_sb3(ppo, MPCEngine(horizon=20, device=0), device=dev)
    elif ppo_random:
        torch.manual_seed(seed)
        agents["ppo"] = rollout.PPOAgent(rollout.ActorCritic(2).to(dev), MPCEngine(horizon=20, device=0))
    return agents, tmp


def add_agent_flags(ap):
    src = ap.add_mutually_exclusive_group()
    src.add_argument("--mpcrl", help="an SB3 checkpoint (.zip) of the reference's MPC-RL agent")
    src.add_argument("--fixture", action="store_true", help="MPC-RL: the v0 PPO policy of tests/golden/sb3_policies.npz")
    base = ap.add_mutually_exclusive_group()
    base.add_argument("--ppo", metavar="PATH", help="the end-to-end PPO baseline: a checkpoint (.zip) as ActorCritic.save_sb3 writes it")
    base.add_argument("--ppo-random", action="store_true", help="the end-to-end PPO baseline with an untrained policy seeded by --seed")


def actuation_of(args):
    """The --act-* flags as evaluate.Actuation's keyword arguments; None when none was given: no actuator model, the launches
    of before"""
    given = dict(delay=args.act_delay, p_hold=args.act_p_hold, limits=args.act_limits,
                 tau=None if args.act_tau_accel is None and args.act_tau_steer is None
                 else (args.act_tau_accel or 0.0, args.act_tau_steer or 0.0),
                 rate=None if args.act_rate_accel is None and args.act_rate_steer is None
                 else (args.act_rate_accel or float("inf"), args.act_rate_steer or float("inf")),
                 sigma=None if args.act_sigma_accel is None and args.act_sigma_steer is None
                 else (args.act_sigma_accel or 0.0, args.act_sigma_steer or 0.0),
                 offset=None if args.act_steer_offset is None else (0.0, args.act_steer_offset))
    given = {k: v for k, v in given.items() if v is not None}
    return dict(given, seed=args.seed) if given else None


def add_actuation_flags(ap):
    ap.add_argument("--act-delay", type=int, metavar="N", help="actuator: transport delay in whole policy steps (0..7)")
    ap.add_argument("--act-tau-accel", type=float, metavar="S", help="actuator: time constant of the acceleration's lag [s]")
    ap.add_argument("--act-tau-steer", type=float, metavar="S", help="actuator: time constant of the steering's lag [s]")
    ap.add_argument("--act-rate-accel", type=float, metavar="R", help="actuator: largest change of the acceleration [m/s^3]")
    ap.add_argument("--act-rate-steer", type=float, metavar="R", help="actuator: largest steering rate [rad/s]")
    ap.add_argument("--act-sigma-accel", type=float, metavar="S", help="actuator: noise on the acceleration [m/s^2]")
    ap.add_argument("--act-sigma-steer", type=float, metavar="S", help="actuator: noise on the steering [rad]")
    ap.add_argument("--act-p-hold", type=float, metavar="P", help="actuator: probability that a step's command is lost")
    ap.add_argument("--act-steer-offset", type=float, metavar="D", help="actuator: steering calibration offset [rad]")
    ap.add_argument("--act-limits", choices=("env",), help="actuator: saturate at the environment's clamp (+-5 m/s^2, +-pi/4)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--episodes-per-env", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--deterministic", action="store_true", help="MPC-RL acts with the policy's mean")
    ap.add_argument("--traffic", default="constant", choices=("constant", "idm"),
                    help="the other vehicles: constant velocity on the approach lanes, or IDM on turning routes")
    ap.add_argument("--metrics", action="store_true", help="also the safety and comfort metrics (evaluate.DriveMetrics)")
    ap.add_argument("--interaction", action="store_true",
                    help="also the interaction metrics (evaluate.InteractionMetrics): yielding, forced braking, "
                         "post-encroachment time; needs --traffic idm")
    ap.add_argument("--range", type=float, default=float("inf"), help="perception: sensing range [m] (default: unlimited)")
    ap.add_argument("--occlusion", default="off", choices=("off", "vehicles", "buildings"),
                    help="perception: vehicles hide what is behind them; buildings: also the four corner buildings "
                         "(evaluate.corner_buildings)")
    ap.add_argument("--dropout", type=float, default=0.0, help="perception: probability that a visible vehicle is dropped")
    ap.add_argument("--sigma-pos", type=float, default=0.0, help="perception: position noise [m]")
    ap.add_argument("--sigma-vel", type=float, default=0.0, help="perception: velocity noise [m/s]")
    ap.add_argument("--sigma-head", type=float, default=0.0, help="perception: heading noise [rad]")
    ap.add_argument("--track-coast", type=int, metavar="N", help="tracker: steps a vehicle that is not measured is kept (0..200)")
    ap.add_argument("--track-gate", type=float, metavar="G", help="tracker: association gate [m] (default 3)")
    ap.add_argument("--track-alpha-pos", type=float, metavar="A", help="tracker: gain on the measured position, (0, 1]")
    ap.add_argument("--track-alpha-vel", type=float, metavar="A", help="tracker: gain on the measured velocity, (0, 1]")
    add_actuation_flags(ap)
    ap.add_argument("--compensate", action="store_true",
                    help="delay compensation: every agent acts on the scene predicted --act-delay steps ahead through the "
                         "nominal actuator (its lag, rate limit and limits), and --sense-delay steps more for the age of "
                         "the scene; needs an --act-* flag or --sense-delay")
    ap.add_argument("--sense-delay", type=int, metavar="N",
                    help="sensing latency: the agent's pipeline is handed the true scene of N policy steps ago (0..7)")
    add_agent_flags(ap)
    ap.add_argument("--plan", action="store_true",
                    help="also score every MPC agent's plan against what happened (evaluate.PlanMetrics): planned clearance, "
                         "prediction error by lead, replanning jump; with --trace the kept episodes also hold the plans")
    ap.add_argument("--plan-leads", type=int, nargs="+", metavar="H",
                    help="--plan: up to four leads in steps, within the horizon (default 1, N/4, N/2, N)")
    ap.add_argument("--plan-gap", type=float, metavar="M", help="--plan: a planned clearance below it is a conflict (default 2.5 m)")
    ap.add_argument("--trace", metavar="KEEP", help="keep the step-by-step record of episodes (evaluate.EpisodeTrace): failed, all, "
                                                     "or a comma-separated list of collision, truncated, success, unsolved")
    ap.add_argument("--trace-window", type=int, default=200, metavar="W", help="--trace: the last W steps of each kept episode")
    ap.add_argument("--trace-capacity", type=int, default=64, metavar="C", help="--trace: at most C episodes per model")
    ap.add_argument("--trace-dir", default="traces", metavar="DIR", help="--trace: one DIR/<model>.npz per model "
                                                                         "(tools/show_episode.py prints them)")
    args = ap.parse_args()
    if args.interaction and args.traffic != "idm":
        ap.error("--interaction requires --traffic idm")

    import math

    import torch
    from mpc_rl_for_avs_amd import evaluate, rollout

    dev = torch.device("cuda", 0)
    agents, tmp = build_agents(dev, args.seed, args.mpcrl, args.fixture, args.ppo, args.ppo_random)
    make_env = lambda: rollout.SyntheticIntersectionEnv(args.envs, device=dev, seed=args.seed, n_others=4,
                                                         traffic=args.traffic)
    flags = dict(range=args.range, occlusion=args.occlusion, dropout=args.dropout,
                 sigma_pos=args.sigma_pos, sigma_vel=args.sigma_vel, sigma_head=args.sigma_head)
    perception = None                    # no flag given: no perception model, the launches of before
    if flags != dict(range=float("inf"), occlusion="off", dropout=0.0, sigma_pos=0.0, sigma_vel=0.0, sigma_head=0.0):
        perception = dict(range=args.range, occlusion=args.occlusion != "off", p_drop=args.dropout,
                          sigma_pos=args.sigma_pos, sigma_vel=args.sigma_vel, sigma_head=args.sigma_head, seed=args.seed,
                          occluders=evaluate.corner_buildings() if args.occlusion == "buildings" else None)
    finite = lambda v: None if isinstance(v, float) and not math.isfinite(v) else v
    echo = {} if perception is None else dict(perception={k: finite(v) for k, v in flags.items()})
    given = dict(coast=args.track_coast, gate=args.track_gate, alpha_pos=args.track_alpha_pos, alpha_vel=args.track_alpha_vel)
    tracker = {k: v for k, v in given.items() if v is not None} or None        # no flag given: no tracker, the launches of before
    if tracker is not None:
        echo["tracker"] = {k: finite(v) for k, v in evaluate.Tracker(0, dev, "hip", **tracker).config.items() if k in given}
    actuation = actuation_of(args)
    if actuation is not None:
        echo["actuation"] = {k: [finite(x) for x in v] if isinstance(v, tuple) else v for k, v in actuation.items()}
    if args.sense_delay is not None:         # no flag given: no latency stage, the launches of before
        echo["sense_delay"] = args.sense_delay
    if args.compensate and actuation is None and args.sense_delay is None:
        ap.error("--compensate matches the actuator model and the sensing delay: give at least one --act-* flag, such as "
                 "--act-delay, or --sense-delay")
    if args.compensate:
        echo["compensate"] = True
    plan = None                          # no flag given: no plan is asked for, the launches of before
    if args.plan or args.plan_leads or args.plan_gap is not None:
        plan = {k: v for k, v in dict(leads=args.plan_leads and tuple(args.plan_leads), gap=args.plan_gap).items() if v is not None}
        echo["plan"] = {k: list(v) if isinstance(v, tuple) else v for k, v in plan.items()}
    trace = None
    if args.trace:
        keep = args.trace.split(",") if "," in args.trace else args.trace
        trace = dict(keep=keep, window=args.trace_window, capacity=args.trace_capacity, **(dict(plan=True) if plan is not None else {}))
        os.makedirs(args.trace_dir, exist_ok=True)
    for name, agent in agents.items():
        results = {}
        s = evaluate.compare({name: agent}, make_env, args.episodes_per_env, deterministic=args.deterministic,
                             seed=args.seed, metrics=args.metrics, perception=perception,
                             interaction=args.interaction, trace=trace, tracker=tracker, actuation=actuation,
                             plan=plan, compensation=True if args.compensate else None, latency=args.sense_delay,
                             results=results)[name]
        s = {k: finite(v) for k, v in s.items()}
        if trace is not None:
            path = os.path.join(args.trace_dir, f"{name}.npz")
            results[name].traces.save(path)
            s.update(trace_file=path, **{f"trace_{k}": v for k, v in results[name].traces.counts.items() if k != "launches"})
        print(json.dumps(dict(agent=name, traffic=args.traffic, envs=args.envs, episodes_per_env=args.episodes_per_env,
                              **echo, **s)), flush=True)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
