"""The yardstick of tests/test_gpu_consistency.py, checked without a GPU: the distance between the oracle's fp16-emulating and fp32
forms of the two-view consistency gradient, with the forward values pinned (here: to the fp16 form's own stored tensors, on the GPU
to the kernels').  The inputs of tests/consistency_cases.py must not make it degenerate:

  * the two views differ, so the loss and every gradient tensor of the fp32 form are non-zero (a rel-L2 against a zero tensor says
    nothing);
  * every number is finite;
  * no tensor's distance reaches 0.5 -- the GPU bound is max(2e-2, 1.5 x distance), and at 0.75 rel-L2 a gradient with the wrong
    sign on half of its mass would still pass.  (0.5 is reasoning about what a bound can still catch, not a measurement.)
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import consistency_cases as C  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402


@pytest.mark.parametrize("name", list(C.CASES))
def test_yardstick_is_not_degenerate(name):
    cfg = C.CASES[name]
    sd = C.weights(cfg)
    v1, v2 = C.make_views(cfg)
    assert (v1 != v2).mean() > 0.5
    pins = []
    for v in (v1, v2):
        taps = {}
        U.forward(sd, v, cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], training=True, emulate_fp16=True, taps=taps)
        pins.append(taps)
    loss, g16, moving, dist, g32 = C.yardstick(sd, v1, v2, cfg, pins[0], pins[1], loss_scale=32768.0)
    print(f"{name}: loss {loss:.4g}; yardstick max {max(dist.values()):.3g} at {max(dist, key=dist.get)}; "
          f"above 2e-2 / 1.5: { {k: round(v, 4) for k, v in dist.items() if 1.5 * v > 2e-2} }")
    assert np.isfinite(loss) and loss > 0
    for n in g16:
        assert torch.isfinite(g16[n]).all() and torch.isfinite(g32[n]).all(), n
        assert float(g32[n].norm()) > 0 and float(g16[n].norm()) > 0, f"{n}: zero gradient"
        assert dist[n] < 0.5, f"{n}: the fp16 and fp32 forms are {dist[n]:.3g} apart: the bound would check nothing"
    # two sequential momentum updates, view 1 first, are not one update with the mean of the two batches' statistics: the inputs tell
    # the two apart (the GPU test's 1e-5 on the moving statistics would otherwise not see a single averaged update)
    m = U.BN_MOMENTUM
    st = []
    for v in (v1, v2):
        s = {}
        U.forward(sd, v, cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], training=True, emulate_fp16=True, stats_out=s, override=pins[len(st)])
        st.append(s)
    apart = 0.0
    for n, val in moving.items():
        assert torch.isfinite(val).all(), n
        layer, which = n.rsplit(".", 1)
        i = 0 if which == "mean" else 1
        once = sd[n] * m + 0.5 * (st[0][layer][i] + st[1][layer][i]) * (1 - m)
        apart = max(apart, float((val - once).abs().max()))
    assert apart > 1e-4, f"sequential and averaged updates of the moving statistics are only {apart:.3g} apart"
