#!/usr/bin/env python3
"""One calibrate! of the 5-tip clique tree at p = 16 under the PGBP_TUNING of the environment, beliefs and residuals saved as
they come back from the device (run by tests/test_gpu_bs16_planes.py in a child process per tuning: the level, tail and loop
kernels must read and write one and the same packed layout, so the downloads are equal bit for bit).

  python tests/run_bs16_planes_tree.py OUT.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bs16_planes_cases as K  # noqa: E402
import pgbp_amd as P  # noqa: E402


def main():
    prob, packs = K.cliquetree_case(5, 16, 1)
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, np.stack(packs))
    assert P.calibrate_(cgb, prob.schedule, 1, sync=False)[0]
    layout = int(cgb._lib.pgbp_layout(cgb._eng))
    cgb.pull()
    np.savez(sys.argv[1], packed=cgb._packed_raw, res=cgb._res, flags=cgb._flg, layout=layout)
    print("layout", layout)


if __name__ == "__main__":
    main()
