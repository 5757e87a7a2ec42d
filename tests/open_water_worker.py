"""One D8FlowDir + DinfFlowDir call in a process of its own (tests/test_gpu_open_water.py): for the hooks the library reads once per process
(TDX_MACRO_WGS, TDX_LEVELS_LIMIT), which the parent sets in this process's environment.  argv: input .npy (the DEM), output .npz."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == "__main__":
    import taudem_amd

    z = np.load(sys.argv[1])
    with taudem_amd.Context(0) as ctx:
        p, sd8, st = ctx.d8flowdir(z, -3.0e38, 30.0, 30.0, stats=True)
        ang, slp, std = ctx.dinfflowdir(z, -3.0e38, 30.0, 30.0, stats=True)
    np.savez(sys.argv[2], p=p, sd8=sd8, ang=ang, slp=slp, rounds=st["rounds"], levels=st["levels_fall_max"], rounds_dinf=std["rounds"])
