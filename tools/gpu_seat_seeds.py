"""The headline configuration (4096 instances, N = 20, 8 vehicles, collision cost, cap 100) on the seeds 0 .. 7, one process:
per seed the median of 9 timed calls behind 3 warm-up calls, and the iteration counts (to compare two builds' results).
bench.py's headline_over_seeds covers the seeds 0 - 2; profiles/seat_tier.txt is this script, run alternately with two
builds of the library (MPC_EXPERIMENT_LIB=<other build> python tools/gpu_seat_seeds.py parent | python tools/gpu_seat_seeds.py change)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from mpc_rl_for_avs_amd import synth, engine
dev = torch.device('cuda:0')
e = engine.MPCEngine(horizon=20, max_iter=100)
tag = sys.argv[1] if len(sys.argv) > 1 else 'build'
for seed in range(8):
    inp = synth.solver_inputs(4096, 8, seed=seed)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    args = dict(state=t(inp['state'], torch.float64), ego_index=t(inp['ego_index'], torch.int32), weights=t(inp['weights'], torch.float64), is_collide=t(inp['is_collide'], torch.uint8), vref=t(inp['vref'], torch.float64), others=t(inp['others'], torch.float64), collision_cost=True)
    out = e.solve_batch_torch(**args, sync=True)
    for _ in range(2):
        e.solve_batch_torch(**args, out=out, sync=True)
    ts = []
    for _ in range(9):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); e.solve_batch_torch(**args, out=out); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    it = out['iters'].cpu().numpy()
    print(f"{tag} seed {seed}: median {np.median(ts):.4f} ms (min {np.min(ts):.4f} max {np.max(ts):.4f}), at cap {(it>=100).sum()}, iters max {it.max()} sum {it.sum()}", flush=True)
e.close()
