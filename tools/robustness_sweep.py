"""How much latency and actuator lag each model tolerates: the model comparison (evaluate.compare, the agents of
tools/compare_models.py) over a grid of actuator models (evaluate.Actuation) - by default a transport delay of 0, 1, 2, 3
policy steps without lag, then a steering lag of time constant 0, 0.2, 0.5 s without delay - on the same episodes: the same
environment seed in every cell, every agent a fresh environment and a fresh actuator.  Prints one table per model (success
rate, collision rate, mean steps per cell) and one JSON line with every cell's numbers.  --plan also scores every MPC agent's
plan against what happened (evaluate.PlanMetrics) and adds per cell the prediction error at the first and the last lead, the
share of steps with a planned conflict and the replanning jump: whether the plans were bad or the outcome merely left them.
--compensate runs every cell twice on the same episodes, without and with the delay compensator that matches the cell's actuator
(evaluate.Compensation.matching: the agent acts on the scene predicted to the moment its command takes effect), and prints
both rows per model, the compensated one with the compensator's own prediction error; a cell without delay has a look-ahead of
0 steps, for which the compensator hands the scene on unchanged, so its two rows are identical.  The uncompensated rows are
this run's own baseline.
--sense-delay N ... adds a sensing-delay axis (evaluate.Latency: the agents' pipeline is handed the true scene of N policy
steps ago): the grid above is the part with a sensing delay of 0, and every N > 0 is run with each transport delay of
--act-delay (default 0) without lag, as long as their sum is at most 7.  With --compensate the compensator matches both.  When
--check-against names an earlier run's output with the same settings (default profiles/compensation_sweep.txt), the cells
without sensing delay are compared with that run's on every number both hold, and the outcome is printed: they must be equal.

  python tools/robustness_sweep.py --envs 256 --traffic idm --fixture
  python tools/robustness_sweep.py --delays 0 2 4 6 --taus 0 1.0 --act-limits env
  python tools/robustness_sweep.py --envs 256 --traffic idm --fixture --ppo-random --compensate
  python tools/robustness_sweep.py --envs 256 --traffic idm --fixture --ppo-random --sense-delay 0 1 2 3 --act-delay 0 2 --compensate

One run of --envs episodes per cell: a rate carries the sampling noise of that many episodes (at 256, a standard error of up
to 3.1 points), so differences of a few points between cells are within it.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def reproduces(path, settings, table) -> bool:
    """The cells of `table` without sensing delay against the JSON line that ends the earlier run's output at `path`: every
    number both hold of a cell both ran (same model, delay, lag, compensated or not) must be equal.  Prints the outcome; True
    when equal, and when there is nothing to compare with (no file, other settings), which is said too."""
    if not os.path.exists(path):
        print(f"cells without sensing delay: not checked, {path} does not exist")
        return True
    with open(path) as f:
        old = json.loads([line for line in f if line.startswith("{")][-1])
    if any(old.get(k) != v for k, v in settings.items()):
        print(f"cells without sensing delay: not checked, {path} ran with other settings")
        return True
    key = lambda r: (r["delay"], r["tau_steer"], r["compensated"])
    compared, differing = 0, []
    for name, rows in table.items():
        before = {key(r): r for r in old["cells"].get(name, [])}
        for r in rows:
            if r.get("sense_delay", 0) != 0 or key(r) not in before:
                continue
            compared += 1
            differing += [(name, key(r), k) for k, v in before[key(r)].items() if k in r and r[k] != v]
    print(f"cells without sensing delay: {compared} compared with {path}, {len(differing)} numbers differ" +
          "".join(f"\n  {d}" for d in differing[:10]))
    return not differing


def main():
    import compare_models
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--episodes-per-env", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--deterministic", action="store_true", help="MPC-RL acts with the policy's mean")
    ap.add_argument("--traffic", default="idm", choices=("constant", "idm"))
    ap.add_argument("--delays", type=int, nargs="*", default=[0, 1, 2, 3], metavar="N",
                    help="transport delays in policy steps, each without lag")
    ap.add_argument("--taus", type=float, nargs="*", default=[0.0, 0.2, 0.5], metavar="S",
                    help="steering time constants [s], each without delay")
    ap.add_argument("--act-limits", choices=("env",), help="saturate at the environment's clamp in every cell")
    ap.add_argument("--plan", action="store_true", help="also the plan metrics of every MPC agent, per cell")
    ap.add_argument("--compensate", action="store_true",
                    help="every cell also with the delay compensator that matches its actuator; both rows per model")
    ap.add_argument("--sense-delay", type=int, nargs="*", default=[0], metavar="N",
                    help="sensing delays in policy steps; 0 is the grid of --delays and --taus, every other one is run with "
                         "each delay of --act-delay")
    ap.add_argument("--act-delay", type=int, nargs="*", default=[0], metavar="N",
                    help="the transport delays every sensing delay > 0 is combined with (sum at most 7)")
    ap.add_argument("--check-against", default=os.path.join(ROOT, "profiles", "compensation_sweep.txt"), metavar="FILE",
                    help="an earlier run's output whose cells without sensing delay must be reproduced")
    compare_models.add_agent_flags(ap)
    args = ap.parse_args()
    if args.plan and args.compensate:
        ap.error("--plan and --compensate exclude each other: the plan metrics' leads assume a plan that starts now")

    import torch
    from mpc_rl_for_avs_amd import evaluate, rollout

    dev = torch.device("cuda", 0)
    agents, tmp = compare_models.build_agents(dev, args.seed, args.mpcrl, args.fixture, args.ppo, args.ppo_random)
    make_env = lambda: rollout.SyntheticIntersectionEnv(args.envs, device=dev, seed=args.seed, n_others=4,
                                                         traffic=args.traffic)
    cells = [(d, 0.0) for d in args.delays] + [(0, t) for t in args.taus if (0, t) not in [(d, 0.0) for d in args.delays]]
    sensing = sorted(set(args.sense_delay)) != [0]           # no sensing delay asked for: no latency stage, the launches of before
    cells = [(0, d, t) for d, t in cells if 0 in args.sense_delay] + \
        [(s, d, 0.0) for s in sorted(set(args.sense_delay)) if s > 0 for d in args.act_delay if s + d <= 7]
    table = {name: [] for name in agents}
    for sense, delay, tau in cells:
        model = dict(delay=delay, tau=(0.0, tau), limits=args.act_limits, seed=args.seed)
        for compensated in (False, True) if args.compensate else (False,):
            out = evaluate.compare(agents, make_env, args.episodes_per_env, deterministic=args.deterministic, seed=args.seed,
                                   actuation=model, plan=True if args.plan else None,
                                   compensation=True if compensated else None, latency=sense if sense > 0 else None)
            for name, s in out.items():
                table[name].append(dict(**(dict(sense_delay=sense) if sensing else {}),
                                        delay=delay, tau_steer=tau, compensated=compensated, success_rate=s["success_rate"],
                                        collision_rate=s["collision_rate"], avg_steps=s["avg_steps"],
                                        mean_return=s["mean_return"],
                                        act_mean_abs_dev_accel=s["act_mean_abs_dev_accel"],
                                        act_mean_abs_dev_steer=s["act_mean_abs_dev_steer"],
                                        **{k: v if math.isfinite(v) else None for k, v in s.items()
                                           if k.startswith(("pred_err_", "plan", "replan_", "min_plan", "comp_", "sense_"))}))
    for name, rows in table.items():
        print(f"{name}: {args.envs * args.episodes_per_env} episodes per cell, traffic {args.traffic}, seed {args.seed}")
        print(("  sense [steps]" if sensing else "") + "  delay [steps]  tau_steer [s]  success %  collision %  mean steps  mean |applied - command| accel, steer" +
              ("  compensated  prediction error mean, max [m]" if args.compensate else ""))
        for r in rows:
            print((f"  {r['sense_delay']:13d}" if sensing else "") +
                  f"  {r['delay']:13d}  {r['tau_steer']:13.2f}  {r['success_rate']:9.1f}  {r['collision_rate']:11.1f}  "
                  f"{r['avg_steps']:10.1f}  {r['act_mean_abs_dev_accel']:.3f}, {r['act_mean_abs_dev_steer']:.4f}" +
                  ("" if not args.compensate else f"  {'yes' if r['compensated'] else 'no':>11}" +
                   (f"  {r['comp_pos_err_mean']:.2e}, {r['comp_pos_err_max']:.2e}" if r["compensated"] else "")))
        if args.compensate:                  # a look-ahead of 0 steps hands the scene on unchanged: the same episodes, bit for bit
            same = lambda a, b: all(a[k] == b[k] for k in ("success_rate", "collision_rate", "avg_steps", "mean_return",
                                                           "act_mean_abs_dev_accel", "act_mean_abs_dev_steer"))
            zero = [(a, b) for a, b in zip(rows[::2], rows[1::2]) if a["delay"] == 0 and a.get("sense_delay", 0) == 0]
            print(f"  cells without delay identical with and without compensation: {all(same(a, b) for a, b in zero)}"
                  if zero else "  no cell without delay")
        leads = sorted(int(k[len("pred_err_lead"):-len("_mean")]) for k in rows[0] if k.startswith("pred_err_lead"))
        if leads:
            lo, hi = leads[0], leads[-1]
            print(f"  delay [steps]  tau_steer [s]  lead-{lo} error [m]  lead-{hi} error [m]  planned conflict  replan accel, steer  "
                  "plans valid")
            for r in rows:
                print(f"  {r['delay']:13d}  {r['tau_steer']:13.2f}  {r[f'pred_err_lead{lo}_mean']:16.3e}  "
                      f"{r[f'pred_err_lead{hi}_mean']:16.3e}  {r['plan_conflict_frac']:16.4f}  {r['replan_accel_mean']:.3f}, "
                      f"{r['replan_steer_mean']:.4f}  {r['plans_valid_frac']:.4f}")
    settings = dict(envs=args.envs, episodes_per_env=args.episodes_per_env, traffic=args.traffic, seed=args.seed,
                    limits=args.act_limits)
    failed = False
    if sensing and 0 in args.sense_delay:
        failed = not reproduces(args.check_against, settings, table)
    print(json.dumps(dict(**settings, compensate=args.compensate, **(dict(sense_delay=sorted(set(args.sense_delay)),
                                                                           act_delay=args.act_delay) if sensing else {}),
                          cells=table)), flush=True)
    if tmp is not None:
        tmp.cleanup()
    if failed:
        sys.exit("the cells without sensing delay differ from the earlier run's")


if __name__ == "__main__":
    main()
