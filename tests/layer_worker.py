"""Worker of test_layer_edges_gpu.py::test_pinned_wave_counts_in_fresh_processes: PA_TALL_WAVES is read once
per process, so the tails of the sixteen-wave tall_linear (B = 1, 33 on buffer-descriptor loads) and of the
eight-wave tall_wgrad run here, in a process of their own.  Prints one JSON list of verdicts (each with the
wave count the launcher's own decision function reports) as its last line.

    PA_TALL_WAVES=16 python -m tests.layer_worker 16
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(waves):
    assert os.environ.get("PA_TALL_WAVES") == waves, "run with PA_TALL_WAVES=%s" % waves
    import torch

    from pyro_amd import kernels as k
    from tests import layer_edge_cases as L
    dev = torch.device("cuda:0")
    out = []
    for B in (1, 33, 127, 4100):
        for i, (R, C) in enumerate(((4, 31), (16, 128), (32, 32), (100, 100), (100, 8), (128, 100), (128, 128),
                                    (17, 33), (3, 127))):
            for orient in ("fwd", "dx"):
                case = dict(B=B, R=R, C=C, orient=orient, bias=orient == "fwd", sigmoid=False,
                            ymul=orient == "dx" and i % 2 == 0, wkind="slice" if (i + B) % 3 == 0 else "contig",
                            gkind="aligned", scale="none")
                nw = L.linear_case_path(case, L.linear_operands(case, dev))["nw"]
                for ints in (True, False):
                    v = L.run_linear_case(case, dev, ints)
                    v["nw"] = nw
                    out.append(v)
    for B in (1, 15, 16, 17, 130, 4097):
        for i, (R, K) in enumerate(((1, 1), (32, 33), (65, 97), (96, 64), (128, 128), (100, 8))):
            case = dict(B=B, R=R, K=K, ymul=i % 2 == 0, want_bias=i % 3 != 2, scale="none")
            nw = k.tall_wgrad_path(B, R, K)["nw"]
            for ints in (True, False):
                v = L.run_wgrad_case(case, dev, ints)
                v["nw"] = nw
                out.append(v)
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
