"""What the delay compensation costs per step: the graph-replayed step of a PureMPC_Agent evaluation (evaluate.evaluate_agent, one
episode per environment) with a perception model (corner buildings, 5 % dropout, bounded noise) and an actuator model with a
transport delay of --steps policy steps, a steering lag of 0.2 s and the environment's limits (the step of
tools/bench_actuation_cost.py with a delayed actuator), with compensation=True - the matching compensator: one more launch
per step, which rolls the ego through the --steps commands in flight and moves and re-orders the others - against
compensation=None, --runs of each in one process, in both orders (off then on in the even runs, on then off in the odd ones).
The yardstick is the run without the stage in the same process.  With --steps above 0 the compensated agent acts on another
scene, so the two kinds of run see the same first scenes and then different episodes, and under a real delay the
uncompensated agent's solves take longer: the difference is then what compensation does to the whole step, not the price of
its launch.  --steps 0 is the identity - the same episodes, the cost of the launch alone - and --delay 0 keeps the look-ahead
of --steps while the actuator has no delay, which prices the kernel's work on steps whose solves stay comparable.  Prints the
time per step of every run (host clock around the stepping loop, which ends in a synchronise, over the steps taken), both
ranges, the difference of the medians, and the compensator's totals.  --kernel instead times the launch alone, apart from any
agent: 2000 back-to-back launches of the stage on --envs environments of ten rows, six present, for every look-ahead 0..7,
between two device events, after 200 warm-up launches; back-to-back launches overlap their launch latency, so this is the
kernel's own time and a lower bound of what it adds to a step.

  python tools/bench_compensation_cost.py --envs 256 --runs 6
  python tools/bench_compensation_cost.py --envs 256 --runs 6 --steps 0
  python tools/bench_compensation_cost.py --envs 256 --runs 6 --steps 3 --delay 0
  python tools/bench_compensation_cost.py --envs 256 --kernel
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def kernel_alone(torch, evaluate, dev, B, seed, launches=2000, warm=200):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    obs = torch.zeros(B, 10, 8)
    obs[:, :7, 0] = 1.0
    obs[:, :7, 1:5] = torch.rand(B, 7, 4, generator=gen) * 20.0 - 10.0
    obs, out = obs.to(dev), torch.zeros(B, 10, 8, device=dev)
    cmd = (torch.rand(B, 2, generator=gen, dtype=torch.float64) - 0.5).to(dev)
    for steps in range(8):
        stage = evaluate.Compensation(B, dev, "hip", steps=steps, tau=(0.0, 0.2), limits="env")
        stage.apply(obs, out, reset=True)
        for _ in range(warm):
            stage.apply(obs, out, command=cmd)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(launches):
            stage.apply(obs, out, command=cmd)
        t1.record()
        torch.cuda.synchronize(dev)
        print(f"look-ahead {steps}: {t0.elapsed_time(t1) * 1e3 / launches:6.2f} us per launch ({launches} back-to-back launches, "
              f"{B} environments)", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3, help="the actuator's delay and the compensator's look-ahead in policy steps (0..7)")
    ap.add_argument("--delay", type=int, help="the actuator's delay when it is not to be --steps")
    ap.add_argument("--kernel", action="store_true", help="time the stage's launch alone, for every look-ahead")
    ap.add_argument("--traffic", default="idm", choices=("constant", "idm"))
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from mpc_rl_for_avs_amd import evaluate, rollout
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent

    class Env:
        config = {"simulation_frequency": 30, "policy_frequency": 10, "observation": {"vehicles_count": 10}}

    dev = torch.device("cuda", 0)
    if args.kernel:
        return kernel_alone(torch, evaluate, dev, args.envs, args.seed)
    agent = PureMPC_Agent(Env(), dict(horizon=20, render=False, weight_speed=1, weight_control=1, weight_input_diff=1),
                          collision_cost=False)
    perception = dict(occlusion=True, occluders=evaluate.corner_buildings(), p_drop=0.05, sigma_pos=0.2, sigma_vel=0.3,
                      sigma_head=0.02, seed=args.seed)
    actuator = dict(delay=args.steps if args.delay is None else args.delay, tau=(0.0, 0.2), limits="env")
    stage = dict(steps=args.steps, tau=actuator["tau"], limits=actuator["limits"])        # Compensation.matching, but for the delay

    def run(with_stage):
        env = rollout.SyntheticIntersectionEnv(args.envs, device=dev, seed=args.seed, n_others=4, traffic=args.traffic)
        res = evaluate.evaluate_agent(agent, env, 1, seed=args.seed, use_graph=True, perception=dict(perception),
                                      actuation=dict(actuator), compensation=dict(stage) if with_stage else None)
        return res.seconds / res.steps * 1e6, res

    run(False), run(True)                                    # warm-up: allocations, lazy initialisation
    us, steps, totals = {False: [], True: []}, {False: set(), True: set()}, None
    for i in range(args.runs):
        for with_stage in ((False, True), (True, False))[i % 2]:
            t, res = run(with_stage)
            us[with_stage].append(t)
            steps[with_stage].add(res.steps)
            totals = res.compensation if with_stage else totals
            print(f"run {i} compensation={'on ' if with_stage else 'off'} {t:8.1f} us/step  ({res.steps} steps, {args.envs} "
                  "environments)", flush=True)
    median = {}
    for with_stage in (False, True):
        v = sorted(us[with_stage])
        median[with_stage] = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        print(f"compensation={'on ' if with_stage else 'off'} min {v[0]:.1f}  median {median[with_stage]:.1f}  max {v[-1]:.1f} us/step")
    print(f"difference of the medians {median[True] - median[False]:+.1f} us/step (look-ahead {args.steps} steps, actuator delay {actuator['delay']}); steps taken "
          f"without the stage {sorted(steps[False])}, with it {sorted(steps[True])}")
    print(f"compensation totals {totals}")


if __name__ == "__main__":
    main()
