#!/usr/bin/env python3
"""Time mpc_policy_control at every tile size E (environments per workgroup: 1, 2, 4, 8, 16) against mpc_policy_act (A = 2), the
one-workgroup-per-environment kernel it shares its arithmetic with - the measurement behind MPC_POLICY_CONTROL_TILE
(include/mpc_mi355x.h; the table is kept as profiles/ppo_policy_control.txt).

Each variant is --launches back-to-back launches captured as one hipGraph (how the collector and the evaluation run the kernel),
replayed between two device events; the variants are replayed in turn, --repeats times after two warm-up rounds, so that a
drift of the clocks hits all of them alike.  Per variant: median, minimum and maximum microseconds per launch over the repeats;
the spread between repeated runs is (max - min) of the same variant.  The outputs of every tile are compared bit for bit with
mpc_policy_act's before anything is timed.

  python tools/bench_policy_control.py --hidden 64 --envs 256 65536
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILES = (1, 2, 4, 8, 16)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 65536])
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--launches", type=int, default=100, help="launches per graph replay (at least 50)")
    ap.add_argument("--repeats", type=int, default=15)
    a = ap.parse_args()
    if a.launches < 50:
        ap.error("--launches must be at least 50")
    import torch
    from mpc_rl_for_avs_amd import engine, rollout
    dev = torch.device("cuda", 0)
    lib = engine.load_library()
    torch.manual_seed(1234)
    pol = rollout.ActorCritic(2, hidden=a.hidden).to(dev)
    pol.refresh_fused()
    f = pol._fz
    H2 = f["b1"].numel()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    weights = tuple(p(f[k]) for k in ("w1", "b1", "w2", "b2", "wh", "bh", "std", "c0"))
    print(f"# mpc_policy_control by tile E against mpc_policy_act (A = 2), hidden {a.hidden} (2H = {H2}), {torch.cuda.get_device_name(dev)}")
    print(f"# {a.launches} launches per hipGraph replay, {a.repeats} repeats after 2 warm-up rounds, variants replayed in turn; us per launch")
    for B in a.envs:
        obs = torch.randn(B, 10, 8, device=dev)
        z = lambda *sh, dt=torch.float32: torch.zeros(sh, dtype=dt, device=dev)
        step = torch.tensor([3], dtype=torch.int64, device=dev)
        outs = {}

        def launcher(name):
            o = outs[name] = dict(noise=z(B, 2), act=z(B, 2), val=z(B), logp=z(B), rs=z(B, dt=torch.float64), ctrl=z(B, 2, dt=torch.float64))

            def launch():
                stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                if name == "policy_act":
                    rc = lib.mpc_policy_act(dev.index, B, 2, H2, p(obs), *weights, p(o["noise"]), 7, 0, p(step), 0, 1, p(o["act"]),
                                            p(o["val"]), p(o["logp"]), None, p(o["rs"]), stream)
                else:
                    rc = lib.mpc_policy_control_tile(int(name[1:]), dev.index, B, H2, p(obs), *weights, p(o["noise"]), 7, 0, p(step),
                                                     p(o["act"]), p(o["val"]), p(o["logp"]), p(o["ctrl"]), stream)
                if rc != 0:
                    raise RuntimeError(lib.mpc_last_error().decode())
            return launch

        names = ["policy_act"] + [f"E{t}" for t in TILES]
        launch = {n: launcher(n) for n in names}
        graphs = {}
        side = torch.cuda.Stream(dev)
        for n in names:
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                launch[n]()
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(a.launches):
                    launch[n]()
            graphs[n] = g
        torch.cuda.synchronize(dev)
        for n in names[1:]:                    # same bits, or the timing compares different work
            for k in ("noise", "act", "val", "logp"):
                assert torch.equal(outs[n][k], outs["policy_act"][k]), (B, n, k)
        us = {n: [] for n in names}
        for r in range(a.repeats + 2):
            for n in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[n].replay()
                e1.record()
                torch.cuda.synchronize(dev)
                if r >= 2:
                    us[n].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        print(f"\nB = {B}")
        print(f"{'variant':<12}{'median':>10}{'min':>10}{'max':>10}{'spread':>10}")
        for n in names:
            v = sorted(us[n])
            print(f"{n:<12}{v[len(v) // 2]:>10.2f}{v[0]:>10.2f}{v[-1]:>10.2f}{v[-1] - v[0]:>10.2f}")
            print("# " + json.dumps(dict(envs=B, hidden=a.hidden, variant=n, us_median=v[len(v) // 2], us_min=v[0], us_max=v[-1])))


if __name__ == "__main__":
    main()
