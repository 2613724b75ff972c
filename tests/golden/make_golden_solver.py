"""Record tests/golden/solver_golden.npz from the reference's solver (pure torch / numpy, on the CPU):

    python tests/golden/make_golden_solver.py <root of the reference checkout>

  * sched_<case>_lr / _mom [n + 1, G] float64: the groups' learning rate and momentum (beta1 for Adam) after the construction of the
    reference's scheduler and after every iteration, for the cases of tests/solver_oracle.SCHED_CASES;
  * layout_<case>_*: the groups that the reference's make_optimizer builds for tests/solver_oracle.small_model().

The reference's solver/build.py and solver/lr_scheduler.py are loaded from their files as a package of their own, so nothing else of the
reference is imported.  Its make_optimizer puts `uncert` on the GPU with .cuda(): that call is made the identity while it runs.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)

from tests import solver_oracle as SO  # noqa: E402


def load_reference_solver(ref_root):
    d = os.path.join(ref_root, "disprcnn", "solver")
    pkg = importlib.util.spec_from_file_location("ref_solver", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(pkg)
    sys.modules["ref_solver"] = mod
    pkg.loader.exec_module(mod)
    return sys.modules["ref_solver.build"], sys.modules["ref_solver.lr_scheduler"]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    build, sched = load_reference_solver(sys.argv[1])
    out = {}
    for name in SO.SCHED_CASES:
        lr, mom = SO.walk_schedule(name, sched, torch.optim.SGD, torch.optim.Adam)
        out[f"sched_{name}_lr"], out[f"sched_{name}_mom"] = lr, mom
        print(name, lr[:, 0], mom[:, 0])
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for name, over in SO.LAYOUT_CASES.items():
            opt, uncert = build.make_optimizer(SO.solver_cfg(**over), SO.small_model())
            for k, v in SO.layout_of(opt, uncert).items():
                out[f"layout_{name}_{k}"] = v
    finally:
        torch.Tensor.cuda = cuda
    path = os.path.join(HERE, "solver_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
