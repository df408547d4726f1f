"""Child process of tests/test_gpu_rrqr.py: one economic pivoted QR of the matrix in argv[1], outputs to the
.npz argv[2].  The parent sets PTHIP_QR_NO_LDS, which the library reads when it loads."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytensor_amd import ffi  # noqa: E402
from pytensor_amd.executor import HipExecutable  # noqa: E402
from pytensor_amd.ir import Graph  # noqa: E402

assert os.environ.get("PTHIP_QR_NO_LDS"), "the parent sets PTHIP_QR_NO_LDS"
ffi.init(0)
x = np.load(sys.argv[1])
g = Graph(name="one_QR")
ins = [g.new_var(str(x.dtype), (None, None))]
outs = [g.new_var(str(x.dtype), (None, None)), g.new_var(str(x.dtype), (None, None)), g.new_var("int32", (None,))]
g.add_node("QR", {"mode": "economic", "pivoting": True}, ins, outs)
g.inputs, g.outputs = ins, outs
res = HipExecutable(g)(x)
np.savez(sys.argv[2], **{f"out{k}": a for k, a in enumerate(res)})
