"""Print a kept episode of a trace file (evaluate.EpisodeTraces.save; tools/compare_models.py --trace writes one per model) as
a table, one line per kept step: the step number, the ego's pose and speed in the scene the step started from, the action as
commanded, the reward, the solve's status / iterations, the flags (D done, T truncated, C crashed, A arrived) and the centre
distance to the nearest present vehicle (with its row), and a last line for the scene the episode ended in.  With a recorded
`seen` plane the number of rows the agent saw is printed next to the number present.  Without --episode the file's episodes
are listed.  --plan (a trace recorded with plan=True, compare_models.py --plan --trace) adds per step the plan behind the
action: its clearance to where the vehicles of the scene the step started from will be under constant velocity (the smallest
distance over the stages, with the stage), and the plan's end point and end speed.

  python tools/show_episode.py out/pure_mpc.npz
  python tools/show_episode.py out/pure_mpc.npz --episode 3 --plan
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUTCOMES = ((1, "collision"), (2, "truncated"), (4, "success"), (8, "unsolved"))


def outcome_names(bits: int) -> str:
    return "+".join(name for bit, name in OUTCOMES if bits & bit) or "none"


def nearest(scene):
    """(distance, row) of the nearest present vehicle to the ego of scene [R, 8], or (inf, -1)"""
    best = (math.inf, -1)
    for i in range(1, scene.shape[0]):
        if scene[i, 0] != 0:
            d = math.hypot(float(scene[i, 1]) - float(scene[0, 1]), float(scene[i, 2]) - float(scene[0, 2]))
            if d < best[0]:
                best = (d, i)
    return best


def planned_clearance(X, scene, dt):
    """(distance, stage) at which the planned positions X [N + 1, 4] come closest to the present vehicles of scene [R, 8]
    moved on with their velocity, over the stages 1..N; (inf, -1) when no vehicle is present"""
    best = (math.inf, -1)
    for k in range(1, X.shape[0]):
        for i in range(1, scene.shape[0]):
            if scene[i, 0] != 0:
                d = math.hypot(float(X[k, 0]) - (float(scene[i, 1]) + k * dt * float(scene[i, 3])),
                               float(X[k, 1]) - (float(scene[i, 2]) + k * dt * float(scene[i, 4])))
                if d < best[0]:
                    best = (d, k)
    return best


def listing(tr) -> str:
    c = tr.counts
    lines = [f"{len(tr)} episodes kept of {c['matched']} matched ({c['dropped']} dropped), window {tr.window}, "
             f"{c['launches']} launches, recorder memory {tr.nbytes / 2 ** 20:.1f} MiB",
             f"{'episode':>7} {'env':>6} {'ordinal':>7} {'steps':>5} {'first':>5} {'ended on':>8}  outcome"]
    ix = tr.index
    for i in range(len(tr)):
        lines.append(f"{i:>7} {ix['env'][i]:>6} {ix['ordinal'][i]:>7} {ix['steps'][i]:>5} {ix['first'][i]:>5} "
                     f"{ix['launch'][i]:>8}  {outcome_names(int(ix['outcome'][i]))}")
    return "\n".join(lines)


def table(tr, i: int, plan: bool = False, dt: float = 0.1, speed_column: int = 3) -> str:
    e = tr.episode(i)
    if plan and "plan_X" not in e:
        raise SystemExit("--plan: this trace holds no plans (record it with plan=True: compare_models.py --plan --trace ...)")
    L = e["action"].shape[0]
    lines = [f"episode {i}: environment {e['env']}, ordinal {e['ordinal']}, {e['steps']} steps (kept from step {e['first']}), "
             f"ended on launch {e['launch']}: {outcome_names(e['outcome'])}",
             f"{'step':>4} {'x':>8} {'y':>8} {'heading':>7} {'speed':>6} {'accel':>7} {'steer':>7} {'reward':>8} {'status':>6} "
             f"{'iters':>5} {'flags':>5} {'nearest':>8} {'row':>3}" + (f" {'seen':>5}" if "seen" in e else "") +
             (f" {'planned':>8} {'at':>3} {'end x':>8} {'end y':>8} {'end v':>6}" if plan else "")]
    for k in range(L + 1):
        s = e["scene"][k]
        d, row = nearest(s)
        pose = f"{e['first'] + k:>4} {s[0, 1]:>8.2f} {s[0, 2]:>8.2f} {s[0, 5]:>7.3f} {math.hypot(float(s[0, 3]), float(s[0, 4])):>6.2f}"
        near = f"{d:>8.2f} {row:>3}" if row >= 0 else f"{'-':>8} {'-':>3}"
        if k == L:
            lines.append(f"{pose} {'':>7} {'':>7} {'':>8} {'':>6} {'':>5} {'end':>5} {near}")
            break
        f = int(e["flags"][k])
        flags = "".join(c if f & bit else "." for bit, c in ((1, "D"), (2, "T"), (4, "C"), (8, "A")))
        line = (f"{pose} {e['action'][k, 0]:>7.3f} {e['action'][k, 1]:>7.3f} {e['reward'][k]:>8.3f} {e['status'][k]:>6} "
                f"{e['iters'][k]:>5} {flags:>5} {near}")
        if "seen" in e:
            present = int((s[1:, 0] != 0).sum())
            line += f" {int((e['seen'][k][1:, 0] != 0).sum()):>2}/{present:<2}"
        if plan:
            X = e["plan_X"][k]
            c, stage = planned_clearance(X, e["seen"][k] if "seen" in e else s, dt)
            line += (f" {c:>8.2f} {stage:>3}" if stage >= 0 else f" {'-':>8} {'-':>3}") + \
                f" {X[-1, 0]:>8.2f} {X[-1, 1]:>8.2f} {X[-1, speed_column]:>6.2f}"
        lines.append(line)
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file", help="a .npz written by EpisodeTraces.save")
    ap.add_argument("--episode", type=int, help="the kept episode to print (default: list them)")
    ap.add_argument("--plan", action="store_true", help="also the plan behind every action: planned clearance, end point, end speed")
    ap.add_argument("--dt", type=float, default=0.1, help="--plan: the policy step [s]")
    ap.add_argument("--plan-order", type=int, default=0, choices=(0, 1),
                    help="--plan: the plan's state order, 0 x y theta v (NLP agents), 1 x y v yaw (the iterative-linear agent)")
    args = ap.parse_args()
    from mpc_rl_for_avs_amd.evaluate import EpisodeTraces
    tr = EpisodeTraces.load(args.file)
    if args.episode is None:
        print(listing(tr))
    elif not 0 <= args.episode < len(tr):
        ap.error(f"--episode must be 0..{len(tr) - 1}")
    else:
        print(table(tr, args.episode, args.plan, args.dt, 3 if args.plan_order == 0 else 2))


if __name__ == "__main__":
    main()
