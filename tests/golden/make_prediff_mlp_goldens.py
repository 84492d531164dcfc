"""Generate tests/golden/g16_prediff_mlp.npz from the reference's own MLP class and training_step (CPU, fp32).

    python tests/golden/make_prediff_mlp_goldens.py <reference checkout root>

The reference train.py imports pytorch_lightning, omegaconf and wandb at module level, so it is not imported: the `MLP`
class definition and the statements of `Model.training_step` up to the loss are taken out of the file with `ast` at run
time and executed against torch.  Nothing from the reference is copied; the fixture holds inputs and recorded results
only.

Recorded for a seeded batch of B = 2 sequences of 25 frames of 16 x 16 ('NHWT', values in [0, 1]): `batch`, the
ordered state-dict key list `keys` and the seeded initial values `init_<i>`, `x`, `target`, `pred`, `loss`, the
gradients `grad_<i>` and the parameters `post_<i>` after 3 steps of torch.optim.AdamW (lr 1e-3, wd 1e-2) with
clip_grad_norm_(1.0), whose returned norms are `gnorm` (i indexes `keys`).
"""
from __future__ import annotations

import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 1234
B, T, H, W = 2, 25, 16, 16


def load_reference(root):
    """-> (MLP class, step(self, batch) -> dict of the training_step's locals)"""
    path = os.path.join(root, "experiments", "v1_experiments", "prediff_mlp_sevir", "train.py")
    tree = ast.parse(open(path).read(), path)
    mlp = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MLP"]
    model = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Model"]
    assert len(mlp) == 1 and len(model) == 1, path
    step = [n for n in model[0].body if isinstance(n, ast.FunctionDef) and n.name == "training_step"]
    assert len(step) == 1, path
    # the body up to and including `loss = ...`; logging and the return are Lightning's business
    body = []
    for st in step[0].body:
        body.append(st)
        if isinstance(st, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "loss" for t in st.targets):
            break
    else:
        raise AssertionError("training_step assigns no `loss`")
    body.append(ast.Return(value=ast.Call(func=ast.Name(id="locals", ctx=ast.Load()), args=[], keywords=[])))
    fn = ast.FunctionDef(name="step", args=step[0].args, body=body, decorator_list=[], returns=None,
                         type_comment=None, type_params=[])
    mod = ast.fix_missing_locations(ast.Module(body=mlp + [fn], type_ignores=[]))
    ns = {"torch": torch, "nn": nn, "F": F}
    exec(compile(mod, path, "exec"), ns)
    return ns["MLP"], ns["step"]


def main(argv):
    root = argv[1] if len(argv) > 1 else os.environ.get("WFAE_REFERENCE_ROOT")
    if not root:
        raise SystemExit(__doc__)
    MLP, step = load_reference(root)
    torch.manual_seed(SEED)
    net = MLP()
    keys = list(net.state_dict())
    out = {"seed": np.int64(SEED), "keys": np.array(keys)}
    for i, k in enumerate(keys):
        out[f"init_{i}"] = net.state_dict()[k].detach().clone().numpy()
    g = torch.Generator().manual_seed(SEED + 1)
    # blob-like frames: a smooth field per frame plus noise, clipped to [0, 1], so the frame means differ
    level = torch.rand(B, 1, 1, T, generator=g) * 0.5
    batch = (level + 0.3 * torch.rand(B, H, W, T, generator=g)).clamp(0, 1).contiguous()
    out["batch"] = batch.numpy()
    # the reference's `self`: its forward is `self.model(x)`, its criterion nn.MSELoss()
    me = types.SimpleNamespace(input_frames=5, pred_frames=20, model=net, criterion=nn.MSELoss())
    call = type("Self", (), {"__call__": lambda s, x: me.model(x), "__getattr__": lambda s, k: getattr(me, k)})()

    def run():
        return step(call, batch, 0)

    loc = run()
    loc["loss"].backward()
    out["x"] = loc["inp_intensities"].detach().numpy()
    out["target"] = loc["target"].detach().numpy()
    out["pred"] = loc["pred_intensities"].detach().numpy()
    out["loss"] = np.float32(loc["loss"].item())
    params = dict(net.named_parameters())
    for i, k in enumerate(keys):
        out[f"grad_{i}"] = params[k].grad.detach().clone().numpy()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-2)
    net.zero_grad(set_to_none=True)
    norms = []
    for _ in range(3):
        run()["loss"].backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)))
        opt.step()
        opt.zero_grad(set_to_none=True)
    out["gnorm"] = np.array(norms, dtype=np.float32)
    for i, k in enumerate(keys):
        out[f"post_{i}"] = net.state_dict()[k].detach().clone().numpy()
    path = os.path.join(HERE, "g16_prediff_mlp.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv)
