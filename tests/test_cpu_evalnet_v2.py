"""The late-fusion EvalNet (get_evalnet_miou_v2, evalnet.py:76-106) without a GPU: the restatement the GPU tests compare against
(tests/evalnet_v2_cases.py) is itself held to known parameter counts and to a second build of the network from plain torch.nn modules
in float64; three planted defects show that this comparison can tell the rule from its nearest mistakes.  Then the public surface: the
reference's signature (tests/golden/reference_surface_evalnet_v2.json), the repo-root shim, and the drivers' evalnet_arch option, run dry."""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import evalnet_v2_cases as V  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402

# Keras' rule: Conv2D k*k*cin*cout + cout; BatchNormalization 4c, of which gamma and beta (2c) are trainable; Dense cin*units + units.
# By hand for (1, 3, 2), widths 32 / 64 / 128 / 256 and trunk 128 / 256 / 512:
#   input block A  1*32+32 = 64, BN 128                  input block B  3*32+32 = 128, BN 128
#   a tower's blocks  (9*32*32+32) + (32*32+32) + 128 = 10 432;  (9*32*64+64) + (64*64+64) + 256 = 22 912;
#                     (9*64*128+128) + (128*128+128) + 512 = 90 880;  (9*128*256+256) + (256*256+256) + 1024 = 361 984   -> 486 208
#   trunk  (9*256*128+128) + (128*128+128) + 512 = 312 064;  (9*128*256+256) + (256*256+256) + 1024 = 361 984;
#          (9*256*512+512) + (512*512+512) + 2048 = 1 444 864                                                            -> 2 118 912
#   heads  2 * (512*3+3) = 3 078
#   total  64 + 128 + 128 + 128 + 2 * 486 208 + 2 118 912 + 3 078 = 3 094 854;  not trainable: half of every BN's 4c:
#          2 * (32+32+64+128+256) + (128+256+512) = 1 920 channels * 2 = 3 840                                           -> 3 091 014
COUNTS = {(1, 3, 2): (3094854, 3091014), (1, 3, 0.5): (196182, 195222), (3, 9, 1): (780594, 778674), (3, 35, 0.5): (204710, 203750)}


@pytest.mark.parametrize("key", list(COUNTS), ids=[f"ca{k[0]}cb{k[1]}a{k[2]}" for k in COUNTS])
def test_parameter_counts(key):
    ca, cb, alpha = key
    assert V.count_params(ca, cb, cb, alpha) == COUNTS[key]
    table = V.layer_table(ca, cb, cb, alpha)
    assert len(table) == 39
    names = [t[0] for t in table]
    tower = lambda t: [f"{t}.in.c", f"{t}.in.bn"] + [f"{t}{j}.{q}" for j in (1, 2, 3, 4) for q in ("c3", "c1", "bn")]
    assert names == tower("a") + tower("b") + [f"m{i}.{q}" for i in (1, 2, 3) for q in ("c3", "c1", "bn")] + ["iou", "detection"]


# ---- a second opinion: the same network from torch.nn modules, float64, eval mode -----------------------------------------------------
class Second(torch.nn.Module):
    """Built in Keras' creation order from the flat lists of conv and BatchNorm parameters in the restatement's table order, the way
    Keras' own names (conv2d_N, batch_normalization_N) number them.  `defect` plants one mistake."""

    def __init__(self, p, ca, cb, alpha, defect=None):
        super().__init__()
        nn = torch.nn
        table = V.layer_table(ca, cb, cb, alpha)
        convs = iter([(p[n + ".w"], p[n + ".b"]) for n, kind, *_ in table if kind == "conv" and n not in V.HEADS])
        bns = iter([[p[f"{n}.{q}"] for q in ("gamma", "beta", "mean", "var")] for n, kind, *_ in table if kind == "bn"])
        self.defect = defect
        f = lambda v: int(v * alpha)

        def conv(ci, co, k):
            w, b = next(convs)
            m = nn.Conv2d(ci, co, k, padding=k // 2).double()
            if tuple(w.shape) != (k, k, ci, co):
                raise ValueError(f"conv {ci}->{co} k{k} is handed a kernel {tuple(w.shape)}")
            m.weight.data, m.bias.data = w.permute(3, 2, 0, 1).double().contiguous(), b.double()
            return m

        def bnorm(c):
            g, be, mean, var = next(bns)
            m = nn.BatchNorm2d(c, eps=U.BN_EPS).double()
            if g.numel() != c:
                raise ValueError(f"BatchNorm over {c} channels is handed {g.numel()}")
            m.weight.data, m.bias.data, m.running_mean.data, m.running_var.data = g.double(), be.double(), mean.double(), var.double()
            return m

        pool = lambda: nn.MaxPool2d(2, ceil_mode=(defect == "pad"))      # ceil_mode keeps the odd last row / column: Keras 'same' pooling
        block = lambda ci, co: nn.Sequential(conv(ci, co, 3), nn.ReLU(), conv(co, co, 1), nn.ReLU(), bnorm(co), pool())
        stem = lambda ci: nn.Sequential(conv(ci, f(16), 1), nn.ReLU(), bnorm(f(16)))
        widths = [f(16)] + [f(v) for v in V.TOWER]
        blocks = lambda n: [block(widths[j], widths[j + 1]) for j in range(n)]
        if defect == "order":      # tower B's blocks are created before tower A's last block
            a = [stem(ca)] + blocks(3)
            b = [stem(cb)] + blocks(4)
            a.append(block(widths[3], widths[4]))
        else:
            a = [stem(ca)] + blocks(4)
            b = [stem(cb)] + blocks(4)
        self.a, self.b = nn.Sequential(*a), nn.Sequential(*b)
        tw = [widths[4]] + [f(v) for v in V.TRUNK]
        self.trunk = nn.Sequential(*[block(tw[i], tw[i + 1]) for i in range(3)])
        self.heads = [(p[h + ".w"][0, 0].double(), p[h + ".b"].double()) for h in V.HEADS]

    def forward(self, xa, xb):
        a, b = self.a(xa / 255.0), self.b(xb)
        c = torch.cat([a, b], 1)[:, :a.shape[1]] if self.defect == "concat" else a + b
        feat = self.trunk(c).mean(dim=(2, 3))
        return torch.sigmoid(torch.cat([feat @ w + b for w, b in self.heads], 1))


def _weights(ca, cb, alpha, seed):
    """he_normal weights, every bias and BatchNorm statistic perturbed: no parameter sits at a value that hides where it is used"""
    p = V.init_weights(ca, cb, cb, alpha, True, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    for k in p:
        if k.endswith((".b", ".beta", ".mean")):
            p[k] = 0.2 * torch.randn(p[k].shape, generator=gen)
        elif k.endswith((".gamma", ".var")):
            p[k] = 0.5 + torch.rand(p[k].shape, generator=gen)
    return p


SECOND = {"128": dict(h=128, w=128, ca=1, cb=3, alpha=0.5, b=2), "152x208": dict(h=152, w=208, ca=3, cb=5, alpha=0.5, b=2)}
_FIX = {}


def _fixture(name):
    """weights, inputs and the restatement's fp32 output of a case: computed once, shared, left unchanged"""
    if name not in _FIX:
        cfg = SECOND[name]
        p = _weights(cfg["ca"], cfg["cb"], cfg["alpha"], 11)
        xa, xb, _ = V.make_inputs(cfg, 12)
        with torch.no_grad():
            out, _ = V.forward(p, xa, xb, True, True, False)
        _FIX[name] = (cfg, p, xa, xb, out.double().numpy())
    return _FIX[name]


def _second(name, defect=None):
    cfg, p, xa, xb, _ = _fixture(name)
    net = Second(p, cfg["ca"], cfg["cb"], cfg["alpha"], defect).eval()
    with torch.no_grad():
        return net(torch.from_numpy(xa).double().permute(0, 3, 1, 2), torch.from_numpy(xb).double().permute(0, 3, 1, 2)).numpy()


@pytest.mark.parametrize("name", list(SECOND))
def test_restatement_agrees_with_the_torch_nn_build(name):
    want = _fixture(name)[4]
    got = _second(name)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5, np.abs(got - want).max()


@pytest.mark.parametrize("defect,name", [("concat", "128"), ("concat", "152x208"), ("order", "128"), ("order", "152x208"), ("pad", "152x208")])
def test_planted_defects_are_caught(defect, name):
    """each mistake either cannot be built from the parameters in creation order, or moves the outputs far beyond the 1e-5 of the
    comparison above; a fixture that could not tell would fail here"""
    want = _fixture(name)[4]
    try:
        got = _second(name, defect)
    except (ValueError, RuntimeError):
        return
    assert got.shape != want.shape or np.abs(got - want).max() > 1e-3, (defect, np.abs(got - want).max())


def test_the_pad_defect_needs_an_odd_level():
    """at 128 x 128 no level is odd and padding cannot show: the odd case is what catches it"""
    assert np.abs(_second("128", "pad") - _fixture("128")[4]).max() <= 1e-5


def test_fp16_emulation_stays_close_and_the_sum_is_rounded_once():
    cfg, p, xa, xb, want = _fixture("128")
    sums = {}
    with torch.no_grad():
        out, _ = V.forward(p, xa, xb, True, True, False, emulate_fp16=True, sums=sums)
    assert np.abs(out.double().numpy() - want).max() <= 2e-2
    exact = sums["a"].double() + sums["b"].double()
    assert np.array_equal(sums["sum"].numpy(), exact.numpy().astype(np.float16).astype(np.float32))


# ---- the surface -----------------------------------------------------------------------------------------------------------------
def _surface():
    with open(os.path.join(HERE, "golden", "reference_surface_evalnet_v2.json")) as f:
        return json.load(f)


def test_constructor_keeps_the_reference_signature():
    from inconsistencymasks_amd import evalnet as EV
    rec = _surface()
    assert "get_evalnet_miou_v2" in rec["functions"]
    want = rec["signatures"]["get_evalnet_miou_v2"]
    params = list(inspect.signature(EV.get_evalnet_miou_v2).parameters.values())
    got = [[q.name, None if q.default is inspect.Parameter.empty else repr(q.default)] for q in params]
    assert got[:len(want)] == want
    assert [g[0] for g in got[len(want):]] == ["seed", "device", "onehot_B"]      # as get_evalnet_miou
    miou = [q.name for q in inspect.signature(EV.get_evalnet_miou).parameters.values()]
    assert [g[0] for g in got] == miou
    assert "not provided" not in EV.__doc__ and "get_evalnet_miou_v2" in EV.__doc__


def test_root_shim_exports_every_constructor_of_the_reference_module():
    import evalnet as top
    from inconsistencymasks_amd import evalnet as EV
    for name in _surface()["signatures"]:
        assert getattr(top, name) is getattr(EV, name), name


DRY = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
from inconsistencymasks_amd import functions as F, paths, impp_driver, segnet_driver
class Reached(Exception):
    pass
class Net:
    def debug(self, **k): pass
noop = lambda *a, **k: None
for f in dir(F):
    if f.startswith("create_training_data"):
        setattr(F, f, noop)
F.load_model = lambda *a, **k: Net()
which, ds, arch = sys.argv[1:4]
mod = {"impp": impp_driver, "segnet": segnet_driver, "single": segnet_driver}[which]
def ctor(name):
    def call(*a, **k):
        raise Reached(json.dumps([name, [v for v in a], sorted(k)]))
    return call
for name in ("get_evalnet", "get_evalnet_miou", "get_evalnet_miou_v2"):
    setattr(mod, name, ctor(name))
tag = {"HeLa": "HELA", "Cityscapes": "CITYSCAPES"}.get(ds, ds)
os.makedirs(getattr(paths, tag + "_MODEL_DIR"), exist_ok=True)
kw = {} if arch == "default" else {"evalnet_arch": arch}
try:
    if which == "impp":
        impp_driver.run(ds, **kw)
    else:
        segnet_driver.run(ds, ensemble=which == "segnet", **kw)
except Reached as e:
    print("REACHED " + str(e))
except ValueError as e:
    print("REFUSED " + str(e))
"""
CONFIG = """[DEFAULT]
SEED = 42
NUM_EPOCHS = 1
BATCH_SIZE = 8
BATCH_SIZE_EVALNET = 4
NUM_EPOCHS_EVALNET = 1
NUM_LOOPS_TRAIN = 1
NUM_LOOPS_VAL = 1
LR = 0.003
WD = 1e-4
THRESHOLD = 0.4375
TOP_Ks = 2

[{section}]
IMAGE_HEIGHT = 128
IMAGE_WIDTH = 128
IMAGE_CHANNELS = {c}
NUM_CLASSES = {k}
BASE_DIR = {base}/
ALPHA = 0.5
ALPHA_EVALNET = 0.5
ACTIFU = relu
ACTIFU_OUTPUT = sigmoid
MIN_THRESHOLD = 0.25
MAX_THRESHOLD = 0.8125
ERODE_KERNEL = 2
DILATE_KERNEL = 2
BLOCK_INPUT = True
BLOCK_OUTPUT = True
FREE_ROTATION = False
"""


def _dry(tmp_path, which, ds, arch):
    base = str(tmp_path / "data")
    section = {"HeLa": "HELA", "Cityscapes": "CITYSCAPES"}.get(ds, ds)
    cfg = tmp_path / "config.ini"
    cfg.write_text(CONFIG.format(section=section, base=base, c=1 if ds == "HeLa" else 3, k={"ISIC_2018": 1, "HeLa": 3, "SUIM": 8}[ds]))
    env = {**os.environ, "IM_CONFIG": str(cfg), "IM_PARALLEL_CANDIDATES": "1", "WORLD_SIZE": "1", "IM_RUNIDS": "1"}
    r = subprocess.run([sys.executable, "-c", DRY % {"root": ROOT}, which, ds, arch], env=env, capture_output=True, text=True, cwd=tmp_path,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("REACHED ", "REFUSED "))]
    assert lines, r.stdout[-2000:] + r.stderr[-2000:]
    return lines[-1]


@pytest.mark.parametrize("which,ds", [("impp", "HeLa"), ("impp", "SUIM"), ("segnet", "HeLa"), ("segnet", "SUIM"), ("single", "SUIM")])
def test_evalnet_arch_reaches_the_constructor(tmp_path, which, ds):
    for arch, ctor in (("v2", "get_evalnet_miou_v2"), ("default", "get_evalnet_miou")):
        line = _dry(tmp_path, which, ds, arch)
        assert line.startswith("REACHED "), line
        name, args, kwargs = json.loads(line[len("REACHED "):])
        assert name == ctor, line
        assert args == [128, 128, 1 if ds == "HeLa" else 3, 3 if ds == "HeLa" else 8, 0.5], line
        assert ("onehot_B" in kwargs) == (ds == "SUIM") and "seed" in kwargs, line


@pytest.mark.parametrize("which", ["impp", "segnet", "single"])
def test_isic_refuses_v2_by_name(tmp_path, which):
    line = _dry(tmp_path, which, "ISIC_2018", "v2")
    assert line.startswith("REFUSED ") and "ISIC_2018" in line and "v2" in line, line
    line = _dry(tmp_path, which, "ISIC_2018", "default")
    assert line.startswith("REACHED ") and json.loads(line[len("REACHED "):])[0] == "get_evalnet", line
