#!/usr/bin/env python
"""One-off bit dump of a teacher step, to compare two builds of the library in separate, fresh processes:

    python tools/teacher_step_dump.py CASE OUT_DIR [--root TREE]

CASE is a name of tests/teacher_step_cases.py (default, default_shared, four_layers, contact_rows300, ...).  Writes
OUT_DIR/CASE.grad0.npy (the flat gradient of optimizer step 0), CASE.stats.npy (the statistics rows of a whole update) and
CASE.params.npy (the parameters after that update).  --root: the tree whose package and library to load (default: this one)."""
import argparse
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case")
    ap.add_argument("out_dir")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)                          # the cases (tests/teacher_step_cases.py) are this tree's ...
    sys.path.insert(0, os.path.abspath(args.root))    # ... the package and its library --root's
    import numpy as np
    import torch
    import isaacgyminsertion_amd
    from isaacgyminsertion_amd import _lib
    from tests import teacher_step_cases as K
    assert os.path.abspath(isaacgyminsertion_amd.__file__).startswith(os.path.abspath(args.root) + os.sep)
    eng, ro = K.make_engine(K.step_cases()[args.case])
    eng.prepare(ro)
    eng.fwd_bwd(0, 0)
    torch.cuda.synchronize()
    os.makedirs(args.out_dir, exist_ok=True)
    np.save(os.path.join(args.out_dir, args.case + ".grad0.npy"), eng.grads.cpu().numpy())
    stats = eng.update()
    torch.cuda.synchronize()
    np.save(os.path.join(args.out_dir, args.case + ".stats.npy"), stats.cpu().numpy())
    np.save(os.path.join(args.out_dir, args.case + ".params.npy"), eng.params.cpu().numpy())
    print(f"{args.case}: {_lib.lib().igi_build_info().decode()} -> {args.out_dir}")


if __name__ == "__main__":
    main()
