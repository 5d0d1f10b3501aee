"""Generates tests/golden/sb3_policies.npz (run in the build container, where the reference's checkpoints are; the GPU box
only reads the fixture).

The reference ships stable-baselines3 checkpoints of its MPC-RL agents (weights/v0/test_ppo_v0.zip, test_a2c_v0.zip,
weights/v1/test_ppo_v1.zip).  For each, the fixture keeps the tensors of `policy.pth` (read with torch.load(weights_only=True))
as `<name>__<state dict key>` and the `data` JSON as `<name>__data`, with every pickled (`:serialized:`) field reduced to its
`:type:` string - nothing is unpickled.  Tests rebuild a minimal SB3-layout zip from it (tests/test_sde_cpu.py).

The fixtures are data (inputs / expected outputs) only.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("MPC_REFERENCE_DIR", "/root/reference")
CHECKPOINTS = {"ppo_v0": "weights/v0/test_ppo_v0.zip", "a2c_v0": "weights/v0/test_a2c_v0.zip",
               "ppo_v1": "weights/v1/test_ppo_v1.zip"}


def strip_serialized(data):
    return {k: ({":type:": v.get(":type:")} if isinstance(v, dict) and ":serialized:" in v else v) for k, v in data.items()}


def main():
    out = {}
    for name, rel in CHECKPOINTS.items():
        with zipfile.ZipFile(os.path.join(REFERENCE, rel)) as z:
            sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
            data = json.loads(z.read("data").decode("utf-8"))
        for k, v in sd.items():
            out[f"{name}__{k}"] = v.numpy()
        out[f"{name}__data"] = np.array(json.dumps(strip_serialized(data)))
    path = os.path.join(HERE, "sb3_policies.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)", file=sys.stderr)


if __name__ == "__main__":
    main()
