#!/usr/bin/env python3
"""Export the log_std head of the reference's shipped SAC checkpoints (actor.log_std.weight [6][256], actor.log_std.bias [6];
use_sde is False in all four) as plain float32 arrays, next to the actor_*.npz of gen_actor_fixtures.py, which keeps only
latent_pi and mu.

    python tests/golden/gen_log_std_fixtures.py --reference <checkout of the reference>

Source: Trained_Models/Trained_{Ori,Obs,Sta,Dyn}/best_model.zip -> policy.pth, loaded with torch.load(weights_only=True)
(nothing from the file is executed).  Writes tests/golden/actors/log_std_{ori,obs,sta,dyn}.npz with the keys
``log_std_weight`` and ``log_std_bias``: model weights, i.e. data.
"""
import argparse
import io
import os
import zipfile

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    out_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "actors")
    os.makedirs(out_dir, exist_ok=True)
    for name in ("Ori", "Obs", "Sta", "Dyn"):
        z = zipfile.ZipFile(os.path.join(args.reference, "Trained_Models", f"Trained_{name}", "best_model.zip"))
        sd = torch.load(io.BytesIO(z.read("policy.pth")), weights_only=True, map_location="cpu")
        arrs = {k.replace("actor.", "").replace(".", "_"): v.numpy().astype(np.float32)
                for k, v in sd.items() if k.startswith("actor.log_std")}
        assert sorted(arrs) == ["log_std_bias", "log_std_weight"], sorted(arrs)
        np.savez_compressed(os.path.join(out_dir, f"log_std_{name.lower()}.npz"), **arrs)
        print(name, {k: v.shape for k, v in arrs.items()})


if __name__ == "__main__":
    main()
