#!/usr/bin/env python3
"""Export the two Q-networks (critic.qf0, critic.qf1) of the reference's shipped SAC checkpoints as plain float32 arrays, and the
hyperparameters the SAC target needs.

    python tests/golden/gen_critic_fixtures.py [--reference /root/reference] [--out tests/golden/critics]

Source: Trained_Models/Trained_{Ori,Obs,Sta,Dyn}/best_model.zip -> policy.pth and pytorch_variables.pth, loaded with
torch.load(weights_only=True) (nothing from the files is executed), and the JSON member `data` (gamma, tau).  These are DATA files of
the reference (SB3 MultiInputPolicy weights), like tests/golden/gen_actor_fixtures.py exports for the actor.  One file per
Q-network: critics/critic_{ori,obs,sta,dyn}_qf{0,1}.npz with q_{0,2,4}_{weight,bias} = critic.qf{i}.{0,2,4}.{weight,bias}.
critics/sac_hyperparameters.json: gamma, tau and log_ent_coef per checkpoint.

The target networks (critic_target.*) are not exported: they differ from the online ones by Polyak averaging only and would double
the size for no new kernel coverage; tests that need a "target" set use the online one.
"""
import argparse
import io
import json
import os
import zipfile

import numpy as np
import torch

NAMES = ("Ori", "Obs", "Sta", "Dyn")


def export(reference):
    """{file name: {array name: float32 array}}, and the hyperparameters."""
    arrays, hyper = {}, {}
    for name in NAMES:
        z = zipfile.ZipFile(os.path.join(reference, "Trained_Models", f"Trained_{name}", "best_model.zip"))
        sd = torch.load(io.BytesIO(z.read("policy.pth")), weights_only=True, map_location="cpu")
        for i in (0, 1):
            prefix = f"critic.qf{i}."
            arrays[f"critic_{name.lower()}_qf{i}.npz"] = {"q_" + k[len(prefix):].replace(".", "_"): v.numpy().astype(np.float32)
                                                          for k, v in sd.items() if k.startswith(prefix)}
        data = json.loads(z.read("data"))
        var = torch.load(io.BytesIO(z.read("pytorch_variables.pth")), weights_only=True, map_location="cpu")
        hyper[name.lower()] = {"gamma": float(data["gamma"]), "tau": float(data["tau"]), "log_ent_coef": float(var["log_ent_coef"].detach().reshape(-1)[0])}
    return arrays, hyper


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "critics"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    arrays, hyper = export(args.reference)
    for fname, arrs in arrays.items():
        np.savez_compressed(os.path.join(args.out, fname), **arrs)
        print(fname, {k: v.shape for k, v in arrs.items()})
    with open(os.path.join(args.out, "sac_hyperparameters.json"), "w") as f:
        json.dump(hyper, f, indent=1)
    print(hyper)


if __name__ == "__main__":
    main()
