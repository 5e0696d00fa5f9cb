"""GPU tests of the fp32-storage mode of the item encoders (cnn.py ``dtype=torch.float32``, the
models' ``encoder_dtype``): the fp32-MFMA conv tile and the fp32 BatchNorm / pool kernels against
float64 references.  With fp32 storage nothing is rounded to bf16 between layers, so the bounds
here are the fp32 ones (1e-5 per kernel, 1e-4 through the network), not the bf16-emulation bands
of test_gpu_cnn.py."""
import functools

import pytest
import torch
import torch.nn.functional as TF

from oracle import resnet_ref as rref
from oracle import two_tower_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def nrel(a, b):
    """Norm-relative error ||a - b|| / ||b|| (b the float64 reference)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def mrel(a, b):
    """Max-abs error relative to the reference's max-abs."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


# ---------------------------------------------------------------------------- 1. the conv kernel
# (name, cin, Co, k, stride, pad, N, H, W); cin < 8 is zero-padded to C = 8
CONV_GEOMS = [
    ("stem7x7_c1", 1, 64, 7, 2, 3, 3, 17, 23),
    ("stem7x7_c3", 3, 64, 7, 2, 3, 2, 16, 16),
    ("3x3s1_64", 64, 64, 3, 1, 1, 3, 9, 7),
    ("3x3s2_64_128", 64, 128, 3, 2, 1, 2, 9, 10),
    ("1x1s2_64_128", 64, 128, 1, 2, 0, 2, 9, 10),
    ("3x3s1_256_512_tiny", 256, 512, 3, 1, 1, 2, 3, 2),
]
# Bound of every conv check: max-abs error <= CONV_TOL of the float64 result's max-abs.
# torch's own CPU fp32 conv2d (and its autograd) measured against float64 on exactly these
# inputs (conv_case below, tools/fp32_conv_cpu_error.py): worst ratio over the six geometries
#   forward 3.73e-7, dx 4.33e-7, dx + addend 4.19e-7, dW 4.56e-7.
# 4x the worst (1.83e-6) does not exceed 1e-5, so the bound is the 1e-5 stated for this mode; the
# margin covers the kernels' different, but fixed, summation order.
CONV_TOL = 1e-5


def conv_case(name):
    """Inputs and float64 references of one geometry (shared by the checks; never modified)."""
    return _conv_case(name)


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    _, cin, Co, k, s, p, N, H, W = next(g for g in CONV_GEOMS if g[0] == name)
    g = torch.Generator().manual_seed(1000 + len(name) + cin + Co)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(Co, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = torch.randn(N, Co, Ho, Wo, generator=g)
    addend = torch.randn(N, cin, H, W, generator=g)
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    y = TF.conv2d(xd, wd, stride=s, padding=p)
    dx, dw = torch.autograd.grad(y, (xd, wd), dy.double())
    return dict(cin=cin, Co=Co, k=k, s=s, p=p, N=N, H=H, W=W, Ho=Ho, Wo=Wo, x=x, w=w, dy=dy,
                addend=addend, y=y.detach(), dx=dx, dw=dw)


@pytest.mark.parametrize("name", [g[0] for g in CONV_GEOMS])
def test_conv_f32_vs_float64(gpu_pkg, name):
    """ops.conv2d on fp32 tensors (the fp32-MFMA tile): FWD with its BatchNorm column sums,
    DGRAD with and without the addend, WGRAD, each against float64 torch on the CPU at CONV_TOL
    (see its comment for the measured CPU fp32 figures).  The stems' image channels are
    zero-padded to C = 8 (ttmi_nchw_to_nhwc_f32); DGRAD needs Cin == C, so for the stems it is
    checked on the same geometry with the weight zero-padded to 8 input channels — exactly the
    mirror the padded forward multiplies by."""
    ops = gpu_pkg.ops
    c = conv_case(name)
    cin, Co, k, s, p, N, H, W, Ho, Wo = (c[n] for n in ("cin", "Co", "k", "s", "p", "N", "H", "W", "Ho", "Wo"))
    C = max(cin, 8)
    x = torch.empty(N, H, W, C, device=DEV)
    ops.nchw_to_nhwc(c["x"].to(DEV), C, x)
    assert torch.equal(x[..., :cin].cpu(), c["x"].permute(0, 2, 3, 1)) and (x[..., cin:] == 0).all()
    w = c["w"].to(DEV)
    wf = torch.empty(Co, k, k, C, device=DEV)
    ops.conv_weight_prep(w, C, wf, None)
    # FWD + column statistics
    y = torch.empty(N, Ho, Wo, Co, device=DEV)
    cs = torch.zeros(ops.CONV_STAT_REPS * Co, device=DEV, dtype=torch.int64)
    cq = torch.zeros_like(cs)
    ops.conv2d(ops.FWD, N, H, W, C, cin, Co, k, s, p, x=x, w=wf, out=y, colsum=cs, colsumsq=cq)
    y64 = c["y"].permute(0, 2, 3, 1)
    e = {"fwd": mrel(y, y64)}
    s1 = cs.view(ops.CONV_STAT_REPS, Co).sum(0).double().cpu() * 2.0 ** -24
    s2 = cq.view(ops.CONV_STAT_REPS, Co).sum(0).double().cpu() * 2.0 ** -24
    e["colsum"] = mrel(s1, y64.sum((0, 1, 2)))
    e["colsumsq"] = mrel(s2, (y64 * y64).sum((0, 1, 2)))
    # WGRAD (accumulates into torch's [Co, cin, k, k] layout)
    dy = c["dy"].permute(0, 2, 3, 1).contiguous().to(DEV)
    dw = torch.zeros(Co, cin, k, k, device=DEV)
    ops.conv2d(ops.WGRAD, N, H, W, C, cin, Co, k, s, p, x=x, dy=dy, out=dw)
    e["wgrad"] = mrel(dw, c["dw"])
    # DGRAD without / with the addend (Cin == C: the zero-padded weight for the stems)
    w8 = torch.zeros(Co, C, k, k, device=DEV)
    w8[:, :cin] = w
    wf8, wd8 = torch.empty(Co, k, k, C, device=DEV), torch.empty(C, k, k, Co, device=DEV)
    ops.conv_weight_prep(w8, C, wf8, wd8)
    assert torch.equal(wf8, wf)
    dx = torch.full((N, H, W, C), float("nan"), device=DEV)
    ops.conv2d(ops.DGRAD, N, H, W, C, C, Co, k, s, p, dy=dy, w=wd8, out=dx)
    dx64 = c["dx"].permute(0, 2, 3, 1)
    e["dgrad"] = mrel(dx[..., :cin], dx64)
    assert (dx[..., cin:] == 0).all()
    add = torch.zeros(N, H, W, C, device=DEV)
    add[..., :cin] = c["addend"].permute(0, 2, 3, 1).to(DEV)
    dxa = torch.full((N, H, W, C), float("nan"), device=DEV)
    ops.conv2d(ops.DGRAD, N, H, W, C, C, Co, k, s, p, dy=dy, w=wd8, out=dxa, addend=add)
    e["dgrad+addend"] = mrel(dxa[..., :cin], dx64 + c["addend"].permute(0, 2, 3, 1).double())
    torch.cuda.synchronize()
    print("CONV_F32", name, " ".join(f"{k_} {v:.2e}" for k_, v in e.items()))
    bad = {k_: v for k_, v in e.items() if not v <= CONV_TOL}
    assert not bad, (name, bad)


# ---------------------------------------------------------------------------- 2-4. the network
NET_SHAPES = [(1, 33, 47, 3), (1, 64, 96, 4), (3, 64, 64, 4)]        # (in_ch, H, W, N)
NET_TOL = 1e-4
# The gradient of a ReLU network is discontinuous where a pre-activation is zero: an element
# whose BatchNorm output lies within fp32 rounding of 0 takes one gate in float64 and may take
# the other in ANY fp32 evaluation, which moves a whole channel's gradient by O(1).  torch's own
# CPU fp32 run of the oracle shows it: against float64 it sits at 3.9e-6 .. 5.0e-6 (worst
# gradient) on 13 of 15 seeds tried and at 8.9e-3 / 1.4e-2 on the other two, where one gate
# flipped.  A float64-vs-fp32 gradient comparison is therefore only defined on inputs that keep
# every pre-activation away from the kink.  That is a property of the inputs alone, read off
# the float64 oracle (never off the code under test): the seeds below were found by a CPU-only
# search for draws whose smallest |pre-activation| over all 17 ReLUs is >= KINK_MARGIN, and
# net_run asserts it.  KINK_MARGIN = 1e-5 is ~2-10x the fp32 error of an O(1) BatchNorm output
# behind a K <= 4608 dot product (sqrt(K) * 2^-24 = 4e-6 for the deepest convs, 1e-6 for the
# shallow ones that hold most elements).
KINK_MARGIN = 1e-5
NET_SEEDS = {(1, 33, 47, 3): 1001, (1, 64, 96, 4): 1721, (3, 64, 64, 4): 1010}


class _RecordPreact:
    """Records the smallest |x| that torch.nn.functional.relu sees while active."""

    def __enter__(self):
        self.min, self._orig = float("inf"), TF.relu

        def relu(x, *a, **k):
            self.min = min(self.min, float(x.detach().abs().min()))
            return self._orig(x, *a, **k)
        TF.relu = relu
        return self

    def __exit__(self, *exc):
        TF.relu = self._orig


def _fresh_net(pkg, in_ch, P):
    net = pkg.cnn.ResNet18(in_ch, 128, dtype=torch.float32)
    missing, unexpected = net.load_state_dict(P, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return net.to(DEV)


def _gpu_step(net, x, up):
    out = net(x.to(DEV))
    (out * up.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


_RUNS = {}


def net_run(pkg, shape):
    """One train step of the fp32-mode ResNet-18 and of the float64 oracle from the same
    parameters, then one eval forward of each; computed once per shape and shared."""
    if shape in _RUNS:
        return _RUNS[shape]
    in_ch, H, W, N = shape
    g = torch.Generator().manual_seed(NET_SEEDS[shape])
    P = rref.init_resnet18(in_ch, 128, g)
    x = torch.randn(N, in_ch, H, W, generator=g)
    up = torch.randn(N, 128, generator=g)
    x2 = torch.randn(N, in_ch, H, W, generator=g)
    P64 = {k: (v.double().requires_grad_(True) if "running" not in k else v.double().clone())
           for k, v in P.items()}
    with _RecordPreact() as rec:
        o64 = rref.resnet18_forward(P64, x.double(), update_running=True)
    assert o64.dtype == torch.float64
    assert rec.min >= KINK_MARGIN, ("ill-conditioned inputs: a ReLU gate within fp32 rounding of 0", rec.min)
    (o64 * up.double()).sum().backward()
    with torch.no_grad():
        e64 = rref.resnet18_forward(P64, x2.double(), update_running="eval")
    net = _fresh_net(pkg, in_ch, P)
    out, grads = _gpu_step(net, x, up)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net.eval()
    with torch.no_grad():
        ev = net(x2.to(DEV)).clone()
    torch.cuda.synchronize()
    _RUNS[shape] = dict(P=P, x=x, up=up, P64=P64, o64=o64.detach(), e64=e64, out=out, grads=grads,
                        sd=sd, ev=ev, sd_after_eval=dict(net.state_dict()))
    return _RUNS[shape]


@pytest.mark.parametrize("shape", NET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resnet18_f32_vs_float64_oracle(gpu_pkg, shape):
    """ResNet18(dtype=torch.float32), one train step, against oracle.resnet_ref in float64:
    the output, every parameter gradient and every running_mean / running_var within
    ||gpu - f64|| / ||f64|| <= 1e-4; num_batches_tracked == 1.  (The fp32 CPU oracle itself sits
    1.7-2.0e-6 / 3.7-4.5e-6 / 1.0-1.3e-6 from float64 on these three.)

    Measured on an MI355X (worst of the three shapes): output 3.5e-6 (eval mode 1.5e-6); worst
    gradient 8.2e-6 (layer4.1.bn1.weight, 1x64x96; 7.3e-6 and 7.9e-6 on the other two) — the
    deepest convs and their BatchNorms carry the largest relative error, as in the fp32 CPU
    oracle; worst running statistic 2.2e-6 (layer4.1.bn2.running_mean, 1x33x47)."""
    r = net_run(gpu_pkg, shape)
    errs = {"out": nrel(r["out"], r["o64"])}
    for k, gv in r["grads"].items():
        errs["grad " + k] = nrel(gv, r["P64"][k].grad)
    for k, v in r["sd"].items():
        if "running" in k:
            errs[k] = nrel(v, r["P64"][k])
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
    for k, v in errs.items():
        print("NET_F32", shape, k, f"{v:.3e}")
    worst_g = max((v, k) for k, v in errs.items() if k.startswith("grad "))
    worst_r = max((v, k) for k, v in errs.items() if "running" in k)
    print("NET_F32_WORST", shape, f"out {errs['out']:.3e} grad {worst_g[0]:.3e} {worst_g[1]} "
          f"running {worst_r[0]:.3e} {worst_r[1]}")
    assert len(errs) == 1 + 62 + 40            # every parameter and running statistic was compared
    bad = {k: v for k, v in errs.items() if not v <= NET_TOL}
    assert not bad, bad


@pytest.mark.parametrize("shape", NET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resnet18_f32_eval_mode(gpu_pkg, shape):
    """After that step the running statistics are non-trivial: net.eval() on a fresh input
    against the float64 oracle in eval mode (its own float64 running statistics) at 1e-4, and
    the eval forward updates nothing."""
    r = net_run(gpu_pkg, shape)
    e = nrel(r["ev"], r["e64"])
    print("NET_F32_EVAL", shape, f"{e:.3e}")
    assert e <= NET_TOL, e
    for k, v in r["sd"].items():
        assert torch.equal(v, r["sd_after_eval"][k]), k


def test_resnet18_f32_is_bit_reproducible(gpu_pkg):
    """The same step from the same state twice: output and every gradient torch.equal (the
    BatchNorm statistics and backward sums are int64 fixed point, the split weight gradients a
    fixed-order reduction)."""
    shape = (1, 64, 96, 4)
    r = net_run(gpu_pkg, shape)
    out, grads = _gpu_step(_fresh_net(gpu_pkg, shape[0], r["P"]), r["x"], r["up"])
    assert torch.equal(out, r["out"])
    bad = [k for k in grads if not torch.equal(grads[k], r["grads"][k])]
    assert not bad, bad


# ---------------------------------------------------------------------------- 5. tabular
def test_tabular_f32_vs_float64_oracle(gpu_pkg):
    """TabularEncoder(37, 128, dtype=torch.float32) (T = 37: the zero-padded operand path),
    B = 16, dropout off, against oracle.resnet_ref.tabular_forward in float64: output and
    gradients at 1e-4 norm-relative.  mlp.0.bias feeds a train-mode BatchNorm, so its gradient is
    zero in exact arithmetic: bounded absolutely, at the same 1e-4 of max(1, |reference|)."""
    torch.manual_seed(0)
    enc = gpu_pkg.cnn.TabularEncoder(37, 128, dtype=torch.float32).to(DEV)
    enc.mlp[3].p = 0.0
    g = torch.Generator().manual_seed(3)
    x = torch.randn(16, 37, generator=g)
    up = torch.randn(16, 128, generator=g)
    P64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in enc.named_parameters()}
    o64 = rref.tabular_forward(P64, x.double())
    (o64 * up.double()).sum().backward()
    out = enc(x.to(DEV))
    (out * up.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    errs = {"out": nrel(out, o64)}
    for name, p in enc.named_parameters():
        if name == "mlp.0.bias":
            a = p.grad.abs().max().item()
            print("TAB_F32 mlp.0.bias |grad| max", f"{a:.3e}")
            assert a <= NET_TOL * max(1.0, P64[name].grad.abs().max().item()), a
            continue
        errs[name] = nrel(p.grad, P64[name].grad)
    for k, v in errs.items():
        print("TAB_F32", k, f"{v:.3e}")
    bad = {k: v for k, v in errs.items() if not v <= NET_TOL}
    assert not bad, bad


# ---------------------------------------------------------------------------- 6. model and step
def _cfg3_f32(pkg, B=8, L=12, V=211, T=37, mel=(64, 96), cover=(64, 64), seed=0):
    torch.manual_seed(seed)
    m = pkg.TwoTowerModel(with_text=False, vocab_size=V, tabular_input_dim=T, num_genders=3, num_countries=8,
                          max_seq_len=L, user_embedding_dim=128, item_embedding_dim=128,
                          user_dropout=0.0, precomputed_modalities=False,
                          compute_dtype=torch.float32, encoder_dtype=torch.float32).to(DEV)
    m.item_tower.fusion_layer[3].p = 0.0
    m.item_tower.tabular_encoder.mlp[3].p = 0.0
    g = torch.Generator().manual_seed(seed + 1)
    batch = ref.synthetic_batch(B, L, V, num_countries=8, generator=g)
    del batch["target_modal"]
    batch.update(rref.synthetic_items(B, T, mel, cover, generator=g))
    return m, batch


def test_cfg3_f32_loss_vs_oracle(gpu_pkg):
    """cfg 3 with fp32 operands everywhere (compute_dtype and encoder_dtype fp32): the loss
    against the fp32 CPU oracle (built as test_gpu_cnn.test_cfg3_two_tower_vs_oracle builds its
    fp32 one) within the project's 1e-3 parity bar."""
    m, batch = _cfg3_f32(gpu_pkg)
    params = {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
    with torch.no_grad():
        lref = float(ref.two_tower_loss(params, batch, running=None)[0])
    loss = float(m({k: v.to(DEV) for k, v in batch.items()})[0])
    print("CFG3_F32 loss", loss, "oracle", lref, "diff", abs(loss - lref))
    assert abs(loss - lref) <= 1e-3, (loss, lref)


def test_cfg3_f32_train_step_graph_equals_eager_and_learns(gpu_pkg):
    """TrainStep on the fp32-mode model, two steps on one batch: the graph replay and the eager
    schedule give torch.equal losses and parameters, and the loss falls."""
    m1, batch = _cfg3_f32(gpu_pkg, seed=7)
    m2, _ = _cfg3_f32(gpu_pkg, seed=7)
    bd = {k: v.to(DEV) for k, v in batch.items()}
    s1 = gpu_pkg.TrainStep(m1, lr=1e-3, use_graph=True, seed=11)
    s2 = gpu_pkg.TrainStep(m2, lr=1e-3, use_graph=False, seed=11)
    assert s1.enc_dtypes == [torch.float32, torch.float32] and s1.tab_dtype == torch.float32
    la = [float(s1.step(bd)) for _ in range(2)]
    lb = [float(s2.step(bd)) for _ in range(2)]
    torch.cuda.synchronize()
    assert la == lb, (la, lb)                      # bit-equal fp32 losses
    sa, sb = m1.state_dict(), m2.state_dict()
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, bad[:8]
    assert float(la[1]) < float(la[0]), la


def test_cfg3_f32_model_indexes(gpu_pkg):
    """CatalogueIndexer.add on the fp32-mode model fills the rows of target_id (unit rows) and
    no others."""
    m, batch = _cfg3_f32(gpu_pkg, seed=3)
    V = 211
    ids = torch.tensor([5, 9, 17, 33, 64, 100, 150, 210])
    items = {k: batch[k] for k in ("target_audio", "target_image", "target_tabular")}
    items["target_id"] = ids
    ix = gpu_pkg.retrieval.CatalogueIndexer(m, V)
    ix.add(items)
    torch.cuda.synchronize()
    dense = ix.dense.cpu()
    seen = torch.zeros(V, dtype=torch.bool)
    seen[ids] = True
    assert (dense[~seen] == 0).all()
    assert torch.allclose(dense[seen].norm(dim=1), torch.ones(len(ids)), atol=1e-5)
