"""Golden vectors for the student at token widths 64 and 128 (``*_encoding_size``) with heads of 16, 32 and 64 features
from the REFERENCE's own ``MultiModalModel`` (tact.py:214-599) on CPU (build container only): the encoders at another
``latent_dim``, the positional encoding, the transformer decoder at that width (``mha_ff_dim_factor`` 4 and 1) and the
``Linear(S * d, d)`` output stack.

Recipe of make_golden_student_seq.py: O(1)-scale weights (xavier-uniform, biases U(-0.1, 0.1)), dropout zeroed,
``only_bc=True``.  Stored per case: the initial state_dict, the output ``y`` and the gradient of ``sum(w * y)`` for every
parameter, plus -- from a float64 rerun -- the reference's own fp32-vs-fp64 distance per tensor (``*_ref_noise``).
Inputs and ``w`` are NOT stored: ``case_inputs`` draws them from a seeded generator and the test calls it again.
student_wide_keys.json records the names and shapes of each case's state_dict (nothing else).

    python tests/golden/make_golden_student_wide.py  ->  tests/golden/student_wide.npz,
        student_wide.<case>.{init,grad0}.<part>.npz, student_wide_keys.json
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

#        tag             context, tactile, width, heads, layers, ff factor, B, seed
CASES = [("lin_h10_d64", 10, False, 64, 4, 2, 4, 4, 0),      # 10 tokens, heads of 16
         ("tac_lin_d64h2", 1, True, 64, 2, 1, 4, 3, 1),      # 2 tokens (below the register kernels' cap), heads of 32
         ("lin_h3_d128", 3, False, 128, 2, 1, 1, 8, 2)]      # 3 tokens, heads of 64, ff = 128: ff != 4 d
NUM_LIN, NUM_OUT, TAC_W, TAC_H = 15, 6, 32, 64
# init / grad0 arrays of a case are dealt, in state_dict order, into parts of at most this many bytes of array data: a
# case's weights are 0.9 - 1.3 MB and a committed file stays below 1 MiB
PART_BYTES = 600 * 1024
PARTS = {("lin_h10_d64", "init"): 2, ("lin_h10_d64", "grad0"): 2, ("tac_lin_d64h2", "init"): 2, ("tac_lin_d64h2", "grad0"): 2,
         ("lin_h3_d128", "init"): 3, ("lin_h3_d128", "grad0"): 2}


def case_inputs(context, tactile, B, seed):
    """(obs_tactile (B, T, 3, 1, W, H) or None, lin_input (B, T, 15), w (B, 6)) of a case, from its seed."""
    g = torch.Generator().manual_seed(2000 + seed)
    tac = torch.rand(B, context, 3, 1, TAC_W, TAC_H, generator=g) if tactile else None
    lin = torch.randn(B, context, NUM_LIN, generator=g)
    w = torch.randn(B, NUM_OUT, generator=g)
    return tac, lin, w


def model_kwargs(context, tactile, width, heads, layers, factor):
    return dict(context_size=context, num_channels=1, num_lin_features=NUM_LIN, num_outputs=NUM_OUT,
                tactile_encoder="depth", img_encoder="depth", seg_encoder="depth", tactile_encoding_size=width,
                img_encoding_size=width, seg_encoding_size=width, lin_encoding_size=width, mha_num_attention_heads=heads,
                mha_num_attention_layers=layers, mha_ff_dim_factor=factor, include_lin=True, include_img=False,
                include_seg=False, include_tactile=tactile, include_pcl=False, additional_lin=0, only_bc=True, pcl_conf=None)


def _forward_backward(model, tac, lin, w):
    for p in model.parameters():
        p.grad = None
    y = model(tac, None, None, lin_input=lin)
    (y * w).sum().backward()
    return y.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def run_case(out, keys, RefModel, tag, context, tactile, width, heads, layers, factor, B, seed):
    torch.manual_seed(seed)
    model = RefModel(**model_kwargs(context, tactile, width, heads, layers, factor))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                   # O(1)-scale weights
        for m in model.modules():
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.xavier_uniform_(m.weight, generator=g)
                m.bias.uniform_(-0.1, 0.1, generator=g)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    model.train()
    tac, lin, w = case_inputs(context, tactile, B, seed)
    out[f"{tag}/flags"] = np.array([context, int(tactile), width, heads, layers, factor, B, seed], dtype=np.int64)
    keys[tag] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    for k, v in model.state_dict().items():
        out[f"{tag}/init/{k}"] = v.numpy().copy()
    y, grads = _forward_backward(model, tac, lin, w)
    m64 = copy.deepcopy(model).double()
    y64, g64 = _forward_backward(m64, None if tac is None else tac.double(), lin.double(), w.double())
    out[f"{tag}/y"] = y.numpy().copy()
    out[f"{tag}/y_ref_noise"] = np.array((y.double() - y64).abs().max().item(), dtype=np.float64)
    for k, v in grads.items():
        out[f"{tag}/grad0/{k}"] = v.numpy().copy()
        out[f"{tag}/grad0_ref_noise/{k}"] = np.array((v.double() - g64[k]).abs().max().item(), dtype=np.float64)
    print(tag, "tokens", context * (2 if tactile else 1), "params", sum(p.numel() for p in model.parameters()),
          "max|y|", float(y.abs().max()))


def generate():
    """(arrays, {case: [[state_dict key, shape], ...]})"""
    sys.path.insert(0, HERE)
    import ref_harness as rh
    rh.install()
    from algo.models.transformer.tact import MultiModalModel as RefModel  # (reference)
    torch.set_num_threads(1)
    out, keys = {}, {}
    for case in CASES:
        run_case(out, keys, RefModel, *case)
    return out, keys


def split(out):
    """{file name: arrays}: student_wide.npz holds the small arrays; a case's init and grad0 arrays go, in order, into
    numbered parts of at most PART_BYTES of array data each."""
    files = {"student_wide.npz": {}}
    part, used = {}, {}
    for k, v in out.items():
        tag, kind = k.split("/")[:2]
        if kind not in ("init", "grad0"):
            files["student_wide.npz"][k] = v
            continue
        key = (tag, kind)
        if key not in part or used[key] + v.nbytes > PART_BYTES:
            part[key] = part.get(key, -1) + 1
            used[key] = 0
        used[key] += v.nbytes
        files.setdefault(f"student_wide.{tag}.{kind}.{part[key]}.npz", {})[k] = v
    return files


def file_names():
    """The fixture's array files: student_wide.npz and PARTS[case, kind] numbered parts per case and kind."""
    return ["student_wide.npz"] + [f"student_wide.{c[0]}.{kind}.{i}.npz" for c in CASES for kind in ("init", "grad0")
                                   for i in range(PARTS[c[0], kind])]


KEYS_FILE = "student_wide_keys.json"


def load(folder=HERE):
    """All arrays of the fixture, from exactly the files file_names() lists."""
    out = {}
    for name in file_names():
        with np.load(os.path.join(folder, name)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def load_keys(folder=HERE):
    with open(os.path.join(folder, KEYS_FILE)) as f:
        return json.load(f)


if __name__ == "__main__":
    folder = sys.argv[1] if len(sys.argv) > 1 else HERE               # (another folder: the regeneration test)
    arrays, keys = generate()
    for name, part in split(arrays).items():
        path = os.path.join(folder, name)
        np.savez_compressed(path, **part)
        print(f"wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB")
    with open(os.path.join(folder, KEYS_FILE), "w") as f:
        json.dump(keys, f, indent=1)
        f.write("\n")
