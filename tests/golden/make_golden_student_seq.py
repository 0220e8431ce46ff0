"""Golden vectors for the student with an observation HISTORY (context_size > 1) from the REFERENCE's own
``MultiModalModel`` (tact.py:214-599) on CPU (build container only): the per-step reshape / transpose of the tactile
encodings, the 3-D ``lin_input``, the positional encoding over context x modalities tokens, the transformer decoder over
more than 8 tokens and the ``Linear(S * 32, 32)`` output stack.

Set-up as make_golden_student.py: O(1)-scale weights (xavier-uniform, biases U(-0.1, 0.1): the reference's
trunc_normal(0.02) init gives ~1e-6 outputs), dropout zeroed (its RNG stream cannot be reproduced
across devices), ``only_bc=True``.  Stored per case: the initial state_dict, the output ``y`` and the gradient of
``sum(w * y)`` for every parameter, plus -- from a float64 rerun -- the reference's own fp32-vs-fp64 distance per tensor
(``grad0_ref_noise``, as student.npz has it).  Inputs and ``w`` are NOT stored: ``case_inputs`` draws them from a seeded
generator and the test calls it again.

    python tests/golden/make_golden_student_seq.py  ->  tests/golden/student_seq.npz, student_seq.<case>.{init,grad0}.npz
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

#        tag            context, tactile, B, seed
CASES = [("tac_lin_h16", 16, True, 3, 0),      # 32 tokens: the cap
         ("tac_lin_h5", 5, True, 4, 1),        # 10 tokens: a ragged tile
         ("lin_h12", 12, False, 8, 2)]         # lin only: context_size > 1 alone selects the transformer (tact.py:372)
NUM_LIN, NUM_OUT, TAC_W, TAC_H = 15, 6, 32, 64


def case_inputs(context, tactile, B, seed):
    """(obs_tactile (B, T, 3, 1, W, H) or None, lin_input (B, T, 15), w (B, 6)) of a case, from its seed."""
    g = torch.Generator().manual_seed(1000 + seed)
    tac = torch.rand(B, context, 3, 1, TAC_W, TAC_H, generator=g) if tactile else None
    lin = torch.randn(B, context, NUM_LIN, generator=g)
    w = torch.randn(B, NUM_OUT, generator=g)
    return tac, lin, w


def model_kwargs(context, tactile):
    return dict(context_size=context, num_channels=1, num_lin_features=NUM_LIN, num_outputs=NUM_OUT,
                tactile_encoder="depth", img_encoder="depth", seg_encoder="depth", tactile_encoding_size=32,
                img_encoding_size=32, seg_encoding_size=32, lin_encoding_size=32, mha_num_attention_heads=2,
                mha_num_attention_layers=2, mha_ff_dim_factor=4, include_lin=True, include_img=False, include_seg=False,
                include_tactile=tactile, include_pcl=False, additional_lin=0, only_bc=True, pcl_conf=None)


def _forward_backward(model, tac, lin, w):
    for p in model.parameters():
        p.grad = None
    y = model(tac, None, None, lin_input=lin)
    (y * w).sum().backward()
    return y.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def run_case(out, RefModel, tag, context, tactile, B, seed):
    torch.manual_seed(seed)
    model = RefModel(**model_kwargs(context, tactile))
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
    out[f"{tag}/flags"] = np.array([context, int(tactile), B, seed], dtype=np.int64)
    out[f"{tag}/keys"] = np.array(list(model.state_dict().keys()))
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
    sys.path.insert(0, HERE)
    import ref_harness as rh
    rh.install()
    from algo.models.transformer.tact import MultiModalModel as RefModel  # (reference)
    torch.set_num_threads(1)
    out = {}
    for case in CASES:
        run_case(out, RefModel, *case)
    return out


def split(out):
    """{file name: arrays}: fixtures stay below 1 MiB a file, and a tactile case's weights and gradients are ~0.8 MB
    each, so they get a file per case (as teacher_shared_default.{init,grad}.npz); the rest is student_seq.npz."""
    files = {"student_seq.npz": {}}
    for k, v in out.items():
        tag, kind = k.split("/")[:2]
        name = f"student_seq.{tag}.{kind}.npz" if kind in ("init", "grad0") else "student_seq.npz"
        files.setdefault(name, {})[k] = v
    return files


def file_names():
    """The fixture's files: student_seq.npz and one init / grad0 file per case of CASES."""
    return ["student_seq.npz"] + [f"student_seq.{c[0]}.{kind}.npz" for c in CASES for kind in ("init", "grad0")]


def load(folder=HERE):
    """All arrays of the fixture, from exactly the files file_names() lists."""
    out = {}
    for name in file_names():
        with np.load(os.path.join(folder, name)) as z:
            out.update({k: z[k] for k in z.files})
    return out


if __name__ == "__main__":
    folder = sys.argv[1] if len(sys.argv) > 1 else HERE               # (another folder: the regeneration test)
    for name, arrays in split(generate()).items():
        path = os.path.join(folder, name)
        np.savez_compressed(path, **arrays)
        print(f"wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB")
