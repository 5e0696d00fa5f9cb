"""The two kernels every trained parameter passes through at the end of a step, against plain
high-precision references (oracle/optim_ref.py):

  adamw_kernel (ttmi_adamw / ttmi_adamw_fx)            vs torch.optim.AdamW in float64
  wgrad_fold_kernel (ttmi_wgrad_fold + ttmi_fold_desc) vs the sum in float64 / in split order
  adamw_fold_kernel (ttmi_adamw_folded[_skip], plans)  vs fold-then-update, bit for bit, and fp64

AdamW's tolerance is measured, not fixed: torch.optim.AdamW in float32 on the CPU runs the same
step from the same state, and the kernel may be at most 4x as far from the float64 result as that
independent fp32 implementation is, per tensor (the update p - p_before, m, v).  Every such
comparison prints its figures (``ADAMW_ERR ...``; run with -s to see them).

Folds are exact where the contract says so: int64 fixed-point partials for any S and fp32
partials for S <= 16 equal the in-order float32 restatement bit for bit; fp32 partials for
S > 16 are summed by partitions (include/ttmi.h), checked to 2e-6·Σ|partials| and for run-to-run
bit identity.  The fused tests use integer-valued partials, so the folded gradient is the same
number in fp32 and fp64 and the update's tolerance is the plain update's."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import optim_ref as oref

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
SHIFT = 36                       # TTMI_FX_GRAD_SHIFT
HYPERS = oref.HYPERS
POISON = 12345.0                 # fp32 cells nothing may read or write
POISON_Q = 0x5A5A5A5A5A5A        # the same for int64 cells
F32 = np.float32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).clone().to(DEV)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits16(t):
    return t.detach().cpu().view(torch.int16).numpy().copy()


def _bf16_bits(p):
    return torch.from_numpy(np.ascontiguousarray(p)).to(torch.bfloat16).view(torch.int16).numpy()


def _same(a, b):
    """Bit equality of two arrays (so -0.0 != 0.0 and NaNs compare by payload)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------ AdamW helpers
def _torch32_step(p, g, m, v, hyper, t):
    """One step of torch.optim.AdamW in float32 on the CPU from the given state (step count t - 1
    before it): the independent fp32 implementation that sets the tolerance."""
    lr, b1, b2, eps, wd = hyper
    w = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.AdamW([w], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    st = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()),
          "exp_avg_sq": torch.from_numpy(v.copy())}
    opt.state[w] = st
    w.grad = torch.from_numpy(g.copy())
    opt.step()
    assert float(st["step"]) == t
    return w.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def _assert_step_close(tag, before, g, after, hyper, t, keep=None):
    """``after`` (the kernel's p, m, v) against one float64 AdamW step from ``before`` with the
    gradient ``g``: per tensor at most 4x the max-abs error of torch's float32 CPU step.  ``keep``
    (bool mask) restricts the comparison.  Returns {tensor: (cpu error, kernel error)}."""
    p0, m0, v0 = (np.asarray(x, dtype=F32) for x in before)
    g = np.asarray(g, dtype=F32)
    r = oref.adamw_step64(p0, g, m0, v0, hyper, t)
    c = _torch32_step(p0, g, m0, v0, hyper, t)
    sel = slice(None) if keep is None else keep
    p64 = p0.astype(np.float64)
    triples = (("upd", r[0] - p64, c[0].astype(np.float64) - p64, after[0].astype(np.float64) - p64),
               ("m", r[1], c[1].astype(np.float64), after[1].astype(np.float64)),
               ("v", r[2], c[2].astype(np.float64), after[2].astype(np.float64)))
    out, bad = {}, []
    for name, ref, cpu, ker in triples:
        assert np.isfinite(ker[sel]).all(), (tag, name)
        e_cpu = float(np.abs(cpu[sel] - ref[sel]).max(initial=0.0))
        e_ker = float(np.abs(ker[sel] - ref[sel]).max(initial=0.0))
        print(f"ADAMW_ERR {tag} t={t} lr={hyper[0]:.3g} b1={hyper[1]} {name}: cpu={e_cpu:.3e} kernel={e_ker:.3e}")
        out[name] = (e_cpu, e_ker)
        if e_ker > 4.0 * e_cpu:
            bad.append((name, e_cpu, e_ker))
    assert not bad, (tag, t, bad)
    return out


def _rand_state(rng, n):
    p = rng.standard_normal(n).astype(F32)
    m = (0.1 * rng.standard_normal(n)).astype(F32)
    # v >= m², as a second moment is: with v = 0 under m != 0 the step is m/eps, ill-conditioned
    v = (m.astype(np.float64) ** 2 + (0.05 * rng.standard_normal(n)) ** 2).astype(F32)
    return p, m, v


class _State:
    """p, g, m, v, the bf16 mirror (poisoned), hyper and the step count on the device."""

    def __init__(self, p, g, m, v, hyper, t):
        self.n = int(p.size)
        self.p, self.g, self.m, self.v = _dev(p), _dev(g), _dev(m), _dev(v)
        self.mirror = torch.full((self.n,), -3.0, dtype=torch.bfloat16, device=DEV)
        self.hyper = torch.tensor(list(hyper), dtype=torch.float64, device=DEV)
        self.step = torch.tensor([t], dtype=torch.int32, device=DEV)

    def pmv(self):
        return _np(self.p), _np(self.m), _np(self.v)

    def ptrs(self):
        return (self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                self.mirror.data_ptr(), self.hyper.data_ptr(), self.step.data_ptr())

    def mirror_ok(self):
        return _same(_bits16(self.mirror), _bf16_bits(_np(self.p)))


def _raise_flag(ops):
    """Raise an id_err flag the way a lookup does: a catalogue row whose id is outside the table."""
    x = torch.ones(2, 8, device=DEV)
    ids = torch.tensor([1, 99], dtype=torch.int64, device=DEV)
    ops.catalogue_rows(x, ids, torch.zeros(4, 8, device=DEV))
    assert _np(ops.id_err_flags(x)).any()


def _clear_flags(ops):
    """Clear both halves: the host half by the raising check, the device half by the step reset."""
    t = torch.empty(1, device=DEV)
    try:
        ops.check_id_errors(sync=True)
    except IndexError:
        pass
    dst, src = ops.id_err_step_reset(t)
    ops.batch_copy([dst], [src])
    assert not _np(ops.id_err_flags(t)).any()


# ------------------------------------------------------------ 2. ttmi_adamw / ttmi_adamw_fx
SIZES = [1, 3, 4, 5, 2048, 2052, 10007]   # tail only; 4 | n; one block of 512 float4 groups; +1 group


@pytest.mark.parametrize("t0", [0, 999])
@pytest.mark.parametrize("hi", range(len(HYPERS)))
@pytest.mark.parametrize("n", SIZES)
def test_adamw_against_fp64(gpu_pkg, n, hi, t0):
    """Three steps from non-zero moments with a learning rate rewritten on the device between
    steps; after every step the update, m and v against float64, the mirror, g and the counter.

    The kernel forms m and v in the rounding order of torch's own kernels (ttmi_common.h,
    adam_upd), so on those two it lands on torch's float32 result; with 1 to 5 elements, where
    torch's error is often a few 1e-9 by luck, nothing else could stay within 4x of it.
    Measured on the MI355X (max-abs error against float64; CPU fp32 / kernel), n >= 2048:
      {1e-3, (0.9, 0.999), 1e-8, 0.01}  upd 3.41e-7 / 3.41e-7   m 3.87e-8 / 3.87e-8   v 1.42e-8 / 1.42e-8
      {1e-4, (0.9, 0.999), 1e-8, 0}     upd 2.36e-7 / 2.36e-7   m 3.28e-8 / 3.28e-8   v 1.56e-8 / 1.56e-8
      {3e-2, (0.5, 0.9),   1e-3, 0.1}   upd 2.95e-7 / 2.95e-7   m 1.49e-7 / 1.49e-7   v 1.67e-7 / 1.67e-7
    (the worst kernel/CPU ratio of any tensor at any size and step is 1.00)."""
    ops = gpu_pkg.ops
    hyper = list(HYPERS[hi])
    rng = np.random.default_rng(100000 * hi + 10 * n + (t0 > 0))
    p, m, v = _rand_state(rng, n)
    st = _State(p, np.zeros(n, F32), m, v, hyper, t0)
    for k in range(3):
        t = t0 + k + 1
        hyper[0] = HYPERS[hi][0] * (1.0, 0.5, 2.0)[k]
        st.hyper[0] = hyper[0]                         # the live learning rate
        g = rng.standard_normal(n).astype(F32)
        g[(np.arange(n) + k) % 3 == 0] = 0.0           # gradients that are exactly zero
        before = st.pmv()
        st.g.copy_(torch.from_numpy(g))
        zero_grad = k != 1
        ops.step_inc(st.step)
        ops.adamw(st.p, st.g, st.m, st.v, st.mirror, st.hyper, st.step, zero_grad=zero_grad)
        assert int(st.step) == t                       # read, not written
        _assert_step_close(f"adamw h{hi} n={n}", before, g, st.pmv(), hyper, t)
        assert st.mirror_ok()
        assert _same(_np(st.g), np.zeros(n, F32) if zero_grad else g)
        assert _same(_np(st.hyper), np.array(hyper))


FX_N = 4102                                  # n % 4 = 2: the float4 part ends at 4100
FX_CASES = {"start": (0, 64), "end": (FX_N - FX_N % 4 - 64, 64), "straddle": (2048 - 32, 64), "empty": (400, 0)}


def _fx_setup(seed, off, cnt, hyper, t):
    rng = np.random.default_rng(seed)
    p, m, v = _rand_state(rng, FX_N)
    g = rng.standard_normal(FX_N).astype(F32)
    q = rng.integers(-(1 << 38), 1 << 38, size=cnt + 4, dtype=np.int64)
    q[:cnt][::7] = 0
    q[:cnt][1::7] >>= 26                     # tiny gradients too (a few thousand units of 2^-36)
    g_eff = g.copy()
    g_eff[off:off + cnt] = np.ldexp(q[:cnt].astype(np.float64), -SHIFT).astype(F32)
    g_in = g.copy()
    g_in[off:off + cnt] = POISON             # must not be read
    return (p, m, v), g_in, g_eff, q, _State(p, g_in, m, v, hyper, t)


@pytest.mark.parametrize("hi", range(len(HYPERS)))
@pytest.mark.parametrize("case", sorted(FX_CASES))
def test_adamw_fx_range(gpu_pkg, case, hi):
    """The gradient of [fx_off, fx_off + fx_len) comes from the int64 accumulator at shift 36:
    exactly float32(float64(q)·2^-36), g's poison there unread and left, the accumulator cleared."""
    ops, lib = gpu_pkg.ops, gpu_pkg.lib
    off, cnt = FX_CASES[case]
    hyper, t = HYPERS[hi], 7
    before, g_in, g_eff, q, st = _fx_setup(31 + hi, off, cnt, hyper, t)
    acc = _dev(q)
    if case == "straddle":                   # the ops route computes the offset from the view
        ops.adamw(st.p, st.g, st.m, st.v, st.mirror, st.hyper, st.step, zero_grad=True,
                  fx=(acc[:cnt], st.g[off:off + cnt]))
    else:
        lib.call("ttmi_adamw_fx", FX_N, *st.ptrs(), 1, acc.data_ptr(), off, cnt, SHIFT, None, _stream())
    after = st.pmv()
    _assert_step_close(f"adamw_fx {case} h{hi}", before, g_eff, after, hyper, t)
    # ... and bit for bit the plain kernel fed the converted values
    ref = _State(*before[:1], g_eff, *before[1:], hyper, t)
    ops.adamw(ref.p, ref.g, ref.m, ref.v, ref.mirror, ref.hyper, ref.step, zero_grad=True)
    for a, b in zip(after, ref.pmv()):
        assert _same(a, b)
    assert st.mirror_ok() and _same(_bits16(st.mirror), _bits16(ref.mirror))
    g_after = _np(st.g)
    want = np.zeros(FX_N, F32)
    want[off:off + cnt] = POISON             # g on the range is left as it was
    assert _same(g_after, want)
    q_after = _np(acc)
    assert not q_after[:cnt].any() and _same(q_after[cnt:], q[cnt:])
    assert int(st.step) == t


def test_adamw_fx_range_updates_the_slot_alone(gpu_pkg):
    """ops.adamw_fx_range: ttmi_adamw_fx on the slot's sub-range; the rest is untouched and the
    returned (offset, length) is what adamw(skip=...) takes."""
    ops = gpu_pkg.ops
    off, cnt = 2048 - 32, 64
    hyper, t = HYPERS[0], 3
    before, g_in, g_eff, q, st = _fx_setup(77, off, cnt, hyper, t)
    acc = _dev(q)
    assert ops.adamw_fx_range(st.p, st.g, st.m, st.v, st.mirror, st.hyper, st.step,
                              (acc[:cnt], st.g[off:off + cnt]), zero_grad=True) == (off, cnt)
    after = st.pmv()
    inside = np.zeros(FX_N, bool)
    inside[off:off + cnt] = True
    _assert_step_close("adamw_fx_range", before, g_eff, after, hyper, t, keep=inside)
    for a, b in zip(after, before):
        assert _same(a[~inside], b[~inside])
    assert _same(_np(st.g), g_in)            # the slot's g is not the gradient: left alone
    assert not _np(acc)[:cnt].any()
    mir = _bits16(st.mirror)
    assert _same(mir[inside], _bf16_bits(after[0])[inside])
    assert _same(mir[~inside], _bits16(torch.full((FX_N,), -3.0, dtype=torch.bfloat16))[~inside])


@pytest.mark.parametrize("with_fx", [False, True])
def test_adamw_skip_if(gpu_pkg, with_fx):
    """skip_if with a flag raised: p, m, v and the mirror bit-unchanged, g and the accumulator
    still cleared; with the flags clear the update is the normal one."""
    ops, lib = gpu_pkg.ops, gpu_pkg.lib
    off, cnt = (2048 - 32, 64) if with_fx else (0, 0)
    hyper, t = HYPERS[0], 5
    before, g_in, g_eff, q, st = _fx_setup(5, off, cnt, hyper, t)
    acc = _dev(q)
    flags = ops.id_err_ptr(st.p)
    args = (1, acc.data_ptr() if with_fx else None, off, cnt, SHIFT if with_fx else 0)
    mirror0 = _bits16(st.mirror)
    want_g = np.zeros(FX_N, F32)
    want_g[off:off + cnt] = POISON
    try:
        _raise_flag(ops)
        lib.call("ttmi_adamw_fx", FX_N, *st.ptrs(), *args, flags, _stream())
        for a, b in zip(st.pmv(), before):
            assert _same(a, b)
        assert _same(_bits16(st.mirror), mirror0)
        assert _same(_np(st.g), want_g)
        assert not _np(acc)[:cnt].any() and _same(_np(acc)[cnt:], q[cnt:])
    finally:
        _clear_flags(ops)
    # flags clear: the normal update (from the same state; the gradient put back)
    st.g.copy_(torch.from_numpy(g_in))
    acc.copy_(torch.from_numpy(q))
    lib.call("ttmi_adamw_fx", FX_N, *st.ptrs(), *args, flags, _stream())
    ref = _State(before[0], g_eff, before[1], before[2], hyper, t)
    ops.adamw(ref.p, ref.g, ref.m, ref.v, ref.mirror, ref.hyper, ref.step, zero_grad=True)
    for a, b in zip(st.pmv(), ref.pmv()):
        assert _same(a, b)
    assert not _same(st.pmv()[0], before[0])
    assert st.mirror_ok() and _same(_np(st.g), want_g)


@pytest.mark.parametrize("off,cnt,shift", [(2, 64, SHIFT), (6, 8, SHIFT), (FX_N - FX_N % 4 - 4, 8, SHIFT),
                                           (0, 64, 0)])
def test_adamw_fx_refusals(gpu_pkg, off, cnt, shift):
    """A misaligned fx_off, a range beyond n - n % 4 and fx_shift 0 are refused; nothing runs."""
    lib = gpu_pkg.lib
    before, g_in, _, q, st = _fx_setup(9, 0, 64, HYPERS[0], 2)
    acc = _dev(q)
    with pytest.raises(lib.TTMIError):
        lib.call("ttmi_adamw_fx", FX_N, *st.ptrs(), 1, acc.data_ptr(), off, cnt, shift, None, _stream())
    # the fused entry point refuses the same ranges before it folds anything (n = 4096 here, a
    # multiple of 4 whose segment the fused form takes: the plain entry point is not reached)
    part = _dev(np.ones(8, F32))
    f = lib.FoldDesc()
    f.part, f.S, f.s_stride, f.M, f.N = part.data_ptr(), 1, 8, 1, 8
    f.C, f.ldc, f.accumulate, f.fx_shift = st.g.data_ptr() + 4 * 3072, 8, 3, 0
    plan = _plan(lib, [f])
    assert plan.n == 1
    with pytest.raises(lib.TTMIError):
        lib.call("ttmi_adamw_folded", 4096, *st.ptrs(), 1, acc.data_ptr(), off, cnt, shift,
                 ctypes.byref(plan), None, _stream())
    for a, b in zip(st.pmv(), before):
        assert _same(a, b)
    assert _same(_np(st.g), g_in) and _same(_np(acc), q) and _same(_np(part), np.ones(8, F32))
    assert _same(_bits16(st.mirror), _bits16(torch.full((FX_N,), -3.0, dtype=torch.bfloat16)))


# ------------------------------------------------------------------------- 3. generic folds
def _fold_array(lib, descs):
    return (lib.FoldDesc * max(len(descs), 1))(*descs)


def _no_wgrads(lib):
    return (ctypes.POINTER(lib.WgradDesc) * 1)()


def _run_folds(lib, descs):
    lib.call("ttmi_wgrad_fold", 0, _no_wgrads(lib), len(descs), _fold_array(lib, descs), _stream())


def _plan(lib, descs):
    plan = lib.FoldPlan()
    lib.call("ttmi_wgrad_batch_plan", 0, _no_wgrads(lib), len(descs), _fold_array(lib, descs),
             ctypes.byref(plan), _stream())
    return plan


class _Fold:
    """One ttmi_fold_desc with its host data.  Slabs sit in a poisoned buffer (the padding of
    s_stride > M·N must survive); C is a poisoned [M, ldc] buffer of its own unless the caller
    points the descriptor elsewhere.  ``exact``: integer-valued partials (multiples of 1/16 in
    fixed point), so every sum is exact in fp32 whatever its order."""

    def __init__(self, rng, S, M, N, ldc, acc, fx, pad=0, exact=False):
        self.S, self.M, self.N, self.ldc, self.acc, self.fx = S, M, N, ldc, acc, fx
        self.MN = M * N
        self.s_stride = self.MN + pad
        if fx:
            self.part0 = np.full(S * self.s_stride, POISON_Q, dtype=np.int64)
            vals = (rng.integers(-64, 65, size=(S, self.MN), dtype=np.int64) << (SHIFT - 4)) if exact else \
                rng.integers(-(1 << 44), 1 << 44, size=(S, self.MN), dtype=np.int64)
        else:
            self.part0 = np.full(S * self.s_stride, POISON, dtype=F32)
            vals = rng.integers(-8, 9, size=(S, self.MN)).astype(F32) if exact else \
                rng.standard_normal((S, self.MN)).astype(F32)
        self.vals = vals
        self.c0 = rng.integers(-8, 9, size=M * ldc).astype(F32) if exact else rng.standard_normal(M * ldc).astype(F32)
        self.fill()

    def fill(self):
        for s in range(self.S):
            self.part0[s * self.s_stride: s * self.s_stride + self.MN] = self.vals[s]

    def upload(self):
        self.part, self.C = _dev(self.part0), _dev(self.c0)
        return self

    def desc(self, lib, C=None, ldc=None):
        f = lib.FoldDesc()
        f.part, f.S, f.s_stride, f.M, f.N = self.part.data_ptr(), self.S, self.s_stride, self.M, self.N
        f.C, f.ldc = (self.C.data_ptr() if C is None else C), (self.ldc if ldc is None else ldc)
        f.accumulate, f.fx_shift = self.acc, self.fx
        return f

    def args(self, c):
        return self.part0, self.S, self.s_stride, self.M, self.N, c, self.acc, self.fx

    def abs_sum(self):
        a = np.abs(self.vals.astype(np.float64)).sum(axis=0).reshape(self.M, self.N)
        return np.ldexp(a, -self.fx) if self.fx else a

    def check_parts(self):
        """accumulate bit 1 zeroes exactly the partials read; everything else is as it was."""
        want = self.part0.copy()
        if self.acc & 2:
            for s in range(self.S):
                want[s * self.s_stride: s * self.s_stride + self.MN] = 0
        assert _same(_np(self.part), want), (self.S, self.M, self.N, self.acc, self.fx)

    def check_own_c(self):
        """The fold's result in its own C buffer; returns the [M, N] result."""
        tag = (self.S, self.M, self.N, self.ldc, self.s_stride, self.acc, self.fx)
        got = _np(self.C).reshape(self.M, self.ldc)
        c0 = self.c0.reshape(self.M, self.ldc)
        assert _same(got[:, self.N:], c0[:, self.N:]), tag        # a strided C's other columns
        got, c = got[:, :self.N], c0[:, :self.N]
        if self.fx or self.S <= 16:
            assert _same(got, oref.fold32_in_order(*self.args(c))), tag
        else:
            err = np.abs(got.astype(np.float64) - oref.fold64(*self.args(c)))
            assert (err <= 2e-6 * self.abs_sum()).all(), (tag, float((err / self.abs_sum()).max()))
        return got


FOLD_S = [1, 2, 16, 17, 32, 33, 229]          # both sides of FOLD_NARROW_S and FOLD_WIDE_S; a LayerNorm sum
FOLD_SHAPES = [(1, 128, 128), (1, 4, 4), (8, 64, 64), (8, 64, 80)]


def _fold_matrix(S, fx):
    rng = np.random.default_rng(1000 * S + fx)
    return [_Fold(rng, S, M, N, ldc, acc, fx, pad=pad)
            for (M, N, ldc) in FOLD_SHAPES for pad in (0, 8) for acc in (0, 1, 2, 3)]


@pytest.mark.parametrize("fx", [0, SHIFT])
@pytest.mark.parametrize("S", FOLD_S)
def test_fold_matrix(gpu_pkg, S, fx):
    """32 folds in one launch: every shape x slab stride x accumulate mode at one S and type."""
    lib = gpu_pkg.lib
    folds = _fold_matrix(S, fx)
    assert len(folds) == 32
    runs = []
    for _ in range(2):
        for f in folds:
            f.upload()
        _run_folds(lib, [f.desc(lib) for f in folds])
        res = []
        for f in folds:
            res.append(f.check_own_c())
            f.check_parts()
        runs.append(res)
    for a, b in zip(*runs):                   # a fixed order for a given S: two runs agree
        assert _same(a, b)


@pytest.mark.parametrize("S,MN", [(40, 66048 + 4), (20, 262144 + 4)])
def test_fold_grid_stride_second_pass(gpu_pkg, S, MN):
    """More units than 1024 blocks finish in one pass (16 a block for S > 32, 64 for 17..32): the
    loop, with its barrier, takes a second, partial pass.  Integer-valued partials: the sum is
    exact, so it equals both restatements whatever the partition order."""
    lib = gpu_pkg.lib
    rng = np.random.default_rng(S)
    f = _Fold(rng, S, 1, MN, MN, 3, 0, exact=True).upload()
    _run_folds(lib, [f.desc(lib)])
    got = _np(f.C).reshape(1, MN)
    c = f.c0.reshape(1, MN)
    want = oref.fold64(*f.args(c))
    assert _same(got, want.astype(F32)) and _same(want.astype(F32).astype(np.float64), want)
    assert _same(got, oref.fold32_in_order(*f.args(c)))
    f.check_parts()


def test_fold_more_than_one_launch(gpu_pkg):
    """33 folds in one call: more than FOLD_SEGS = 32, so two launches."""
    lib = gpu_pkg.lib
    rng = np.random.default_rng(33)
    folds = [_Fold(rng, (2, 17, 40)[i % 3], 1, 8 + 4 * (i % 5), 8 + 4 * (i % 5), i % 4, SHIFT * (i % 2)).upload()
             for i in range(33)]
    _run_folds(lib, [f.desc(lib) for f in folds])
    for f in folds:
        f.check_own_c()
        f.check_parts()


# --------------------------------------------- 4. fused fold + update vs fold, then update
class _World:
    """One flat buffer set p, g, m, v, mirror with fold segments whose C are views into g.
    spec: n; segs = [(off | None, M, N, ldc, S, fx, acc)] (off None: C outside g); fx = (off, len)
    of a fixed-point range in a plain gap; skip = (off, len); flags: pass skip_if; tweak(folds).
    Two worlds built from one spec hold the same host data on separate device buffers."""

    def __init__(self, ops, lib, spec, hyper=HYPERS[0], t=4, seed=0):
        self.ops, self.lib, self.spec, self.hyper, self.t = ops, lib, spec, hyper, t
        n = self.n = spec["n"]
        rng = np.random.default_rng(seed)
        self.before = _rand_state(rng, n)
        g0 = rng.standard_normal(n).astype(F32)
        self.folds = []
        for (off, M, N, ldc, S, fx, acc) in spec["segs"]:
            f = _Fold(rng, S, M, N, ldc, acc, fx, pad=8 * (len(self.folds) % 2), exact=True)
            self.folds.append(f)
            if off is not None:               # integer-valued g under a segment: what bit 0 adds to,
                g0[off:off + (M - 1) * ldc + N] = f.c0[:(M - 1) * ldc + N]   # or poison bit 0 clear ignores
        if spec.get("tweak"):
            spec["tweak"](self.folds)
            for f in self.folds:
                f.fill()
        self.fx, self.skip = spec.get("fx"), spec.get("skip")
        self.q = None
        if self.fx:
            o, c = self.fx
            self.q = rng.integers(-(1 << 38), 1 << 38, size=c + 4, dtype=np.int64)
            g0[o:o + c] = POISON
        self.g0 = g0
        self.st = _State(self.before[0], g0, self.before[1], self.before[2], hyper, t)
        self.acc = _dev(self.q) if self.fx else None
        for f in self.folds:
            f.upload()
        self.flags = ops.id_err_ptr(self.st.p) if spec.get("flags") else None

    def descs(self, idxs=None):
        out = []
        for i in (range(len(self.folds)) if idxs is None else idxs):
            off, f = self.spec["segs"][i][0], self.folds[i]
            out.append(f.desc(self.lib) if off is None else f.desc(self.lib, C=self.st.g.data_ptr() + 4 * off))
        return out

    def expected_gradient(self):
        """(a)'s gradient: the folds applied to g0 in call order, in float64; exact in fp32 by
        construction (asserted).  Also the expected contents of the outside C buffers."""
        g = self.g0.astype(np.float64)
        ext = {}
        for i, ((off, M, N, ldc, S, fx, acc), f) in enumerate(zip(self.spec["segs"], self.folds)):
            if off is None:
                c = f.c0.reshape(M, ldc)[:, :N]
                r = f.c0.reshape(M, ldc).astype(np.float64)
                r[:, :N] = oref.fold64(*f.args(c))
                ext[i] = r.reshape(-1)
                continue
            for mr in range(M):
                lo = off + mr * ldc
                row = oref.fold64(f.part0[mr * N:], S, f.s_stride, 1, N, g[lo:lo + N].reshape(1, N), acc, fx)
                g[lo:lo + N] = row.reshape(-1)
        if self.fx:
            o, c = self.fx
            g[o:o + c] = np.ldexp(self.q[:c].astype(np.float64), -SHIFT).astype(F32)
        g32 = g.astype(F32)
        assert _same(g32.astype(np.float64), g)
        return g32, {i: r.astype(F32) for i, r in ext.items()}

    def _fx_args(self):
        if self.fx:
            return self.acc.data_ptr(), self.fx[0], self.fx[1], SHIFT
        return None, 0, 0, SHIFT

    def run_separate(self):
        """(b): ttmi_wgrad_fold, then ttmi_adamw / ttmi_adamw_fx (around a skipped range: two)."""
        lib, st = self.lib, self.st
        if self.folds:
            _run_folds(lib, self.descs())
        if self.skip:
            o, c = self.skip
            for lo, hi in ((0, o), (o + c, self.n)):
                if hi > lo:
                    lib.call("ttmi_adamw", hi - lo, st.p.data_ptr() + 4 * lo, st.g.data_ptr() + 4 * lo,
                             st.m.data_ptr() + 4 * lo, st.v.data_ptr() + 4 * lo, st.mirror.data_ptr() + 2 * lo,
                             st.hyper.data_ptr(), st.step.data_ptr(), 1, self.flags, _stream())
        else:
            lib.call("ttmi_adamw_fx", self.n, *st.ptrs(), 1, *self._fx_args(), self.flags, _stream())
        return self

    def fused(self, plan):
        """(c): one ttmi_adamw_folded / ttmi_adamw_folded_skip over ``plan`` (None: NULL)."""
        lib, st = self.lib, self.st
        pp = ctypes.byref(plan) if plan is not None else None
        if self.skip:
            lib.call("ttmi_adamw_folded_skip", self.n, *st.ptrs(), 1, None, 0, 0, SHIFT, pp,
                     self.skip[0], self.skip[1], self.flags, _stream())
        else:
            lib.call("ttmi_adamw_folded", self.n, *st.ptrs(), 1, *self._fx_args(), pp, self.flags, _stream())
        return self

    def run_fused(self):
        return self.fused(_plan(self.lib, self.descs()))

    def result(self):
        p, m, v = self.st.pmv()
        return {"p": p, "m": m, "v": v, "mirror": _bits16(self.st.mirror)}

    def check_after(self, updated=True):
        """What every path leaves behind: g zero (zero_grad) but for the fixed-point range (left as
        it was) and the skipped range; consumed partials zero, the others intact; the accumulator
        cleared; the mirror bf16(p) where updated; outside C buffers folded."""
        want = np.zeros(self.n, F32)
        keep = np.ones(self.n, bool)
        if self.fx:
            want[self.fx[0]:self.fx[0] + self.fx[1]] = POISON
        if self.skip:
            o, c = self.skip
            want[o:o + c] = self.g0[o:o + c]
            keep[o:o + c] = False
        assert _same(_np(self.st.g), want)
        for f in self.folds:
            f.check_parts()
        if self.fx:
            qa = _np(self.acc)
            assert not qa[:self.fx[1]].any() and _same(qa[self.fx[1]:], self.q[self.fx[1]:])
        g32, ext = self.expected_gradient()
        for i, r in ext.items():
            assert _same(_np(self.folds[i].C), r)
        res = self.result()
        for a, b in zip((res["p"], res["m"], res["v"]), self.before):
            assert _same(a[~keep], b[~keep])                  # the skipped range: bit-unchanged
        poison = _bits16(torch.full((self.n,), -3.0, dtype=torch.bfloat16))
        assert _same(res["mirror"][~keep], poison[~keep])
        if updated:
            assert _same(res["mirror"][keep], _bf16_bits(res["p"])[keep])
            _assert_step_close(self.spec["name"], self.before, g32, (res["p"], res["m"], res["v"]),
                               self.hyper, self.t, keep=keep)
        else:                                                 # skip_if raised: nothing but g and partials
            for a, b in zip((res["p"], res["m"], res["v"]), self.before):
                assert _same(a, b)
            assert _same(res["mirror"], poison)
        return res


def _check_pair(ops, lib, spec, **kw):
    """(c) == (b) bit for bit on p, m, v and the mirror; (b) within the plain update's tolerance of
    (a); both leave g, the partials and the accumulator as the contract says."""
    b = _World(ops, lib, spec, **kw).run_separate()
    c = _World(ops, lib, spec, **kw).run_fused()
    rb = b.check_after()
    rc = c.check_after()
    for k in rb:
        assert _same(rb[k], rc[k]), (spec["name"], k)
    assert not _same(rb["p"], b.before[0])
    return b, c


N4 = 8192


def _overlap_tweak(folds):
    folds[1].vals[:, :128] = folds[0].vals[:, 128:]      # the two agree where they overlap


# segs: (off, M, N, ldc, S, fx, acc)
FUSED = [
    # at the start, adjacent, one float4 apart, a poisoned accumulate-0 destination, at the end
    dict(name="mixed", n=N4, segs=[(0, 1, 256, 256, 1, SHIFT, 3), (256, 1, 128, 128, 16, 0, 1),
                                   (388, 1, 64, 64, 17, 0, 0), (1000, 1, 32, 32, 17, SHIFT, 1),
                                   (2000, 1, 48, 48, 40, SHIFT, 2), (N4 - 512, 1, 512, 512, 40, 0, 3)]),
    dict(name="rows", n=N4, segs=[(64, 8, 64, 64, 16, 0, 3), (576, 4, 32, 32, 17, 0, 1), (704, 2, 8, 8, 40, 0, 3)]),
    # plain gaps of exactly one block of 1024 float4 and of one block plus one unit (AF_U = 4)
    dict(name="gap1024", n=N4, segs=[(0, 1, 8, 8, 2, 0, 3), (8 + 4096, 1, N4 - 4104, N4 - 4104, 1, 0, 3)]),
    dict(name="gap1025", n=N4, segs=[(0, 1, 8, 8, 2, 0, 3), (8 + 4100, 1, N4 - 4108, N4 - 4108, 2, 0, 1)]),
    # the fixed-point range inside a plain gap: across a block boundary of the gap that starts at
    # 8 (block = 4096 floats), ending at a segment's start, covering a whole gap
    dict(name="fx_midblock", n=N4, segs=[(0, 1, 8, 8, 2, 0, 3), (6000, 1, 64, 64, 17, 0, 3)], fx=(4000, 200)),
    dict(name="fx_to_segment", n=N4, segs=[(0, 1, 8, 8, 2, 0, 3), (6000, 1, 64, 64, 17, 0, 3)], fx=(5000, 1000)),
    dict(name="fx_whole_gap", n=N4, segs=[(0, 1, 8, 8, 2, 0, 3), (72, 1, 8, 8, 40, 0, 1)], fx=(8, 64)),
    dict(name="fx_empty", n=N4, segs=[(16, 1, 8, 8, 2, 0, 3)], fx=(4000, 0)),
    # the skipped range: at offset 0, at the end, touching a segment on either side
    dict(name="skip_start", n=N4, segs=[(1024, 1, 64, 64, 16, 0, 3)], skip=(0, 512)),
    dict(name="skip_end", n=N4, segs=[(1024, 1, 64, 64, 17, 0, 3)], skip=(N4 - 512, 512)),
    dict(name="skip_touching", n=N4, segs=[(1024, 1, 64, 64, 40, 0, 3), (2048, 1, 64, 64, 2, SHIFT, 3)],
         skip=(1088, 960)),
    # layouts the fused form cannot take: fold first, then the plain update
    dict(name="fb_n8190", n=8190, segs=[(0, 1, 64, 64, 16, 0, 3), (4096, 1, 64, 64, 17, 0, 1)]),
    dict(name="fb_n8190_fx", n=8190, segs=[(0, 1, 64, 64, 16, 0, 3)], fx=(4000, 200)),
    dict(name="fb_n8190_skip", n=8190, segs=[(0, 1, 64, 64, 16, 0, 3)], skip=(4000, 200)),
    dict(name="fb_strided_rows", n=N4, segs=[(128, 4, 64, 80, 16, 0, 3), (1024, 1, 64, 64, 17, 0, 1)]),
    dict(name="fb_outside_g", n=N4, segs=[(None, 1, 64, 64, 17, 0, 1), (1024, 1, 64, 64, 2, 0, 3)]),
    # two folds of one launch have no order between them: the overlapping halves hold equal sums
    dict(name="fb_overlap", n=N4, segs=[(0, 1, 256, 256, 2, 0, 0), (128, 1, 256, 256, 2, 0, 0)], tweak=_overlap_tweak),
    dict(name="fb_skip_misfit", n=N4, segs=[(128, 4, 64, 80, 16, 0, 3)], skip=(4096, 64)),
]


@pytest.mark.parametrize("spec", FUSED, ids=[s["name"] for s in FUSED])
def test_fused_fold_update(gpu_pkg, spec):
    _check_pair(gpu_pkg.ops, gpu_pkg.lib, spec, hyper=HYPERS[FUSED.index(spec) % 3], t=2 + FUSED.index(spec))


def test_fused_empty_and_null_plans(gpu_pkg):
    """A plan with n = 0, a NULL plan and a NULL plan around a skipped range: the plain update."""
    ops, lib = gpu_pkg.ops, gpu_pkg.lib
    for name, skip, null in (("plan0", None, False), ("null", None, True), ("null_skip", (512, 1024), True),
                             ("plan0_skip", (0, 64), False)):
        spec = dict(name=name, n=N4, segs=[], skip=skip)
        b = _World(ops, lib, spec).run_separate()
        c = _World(ops, lib, spec)
        plan = None if null else lib.FoldPlan()
        assert null or plan.n == 0
        c.fused(plan)
        rb, rc = b.check_after(), c.check_after()
        for k in rb:
            assert _same(rb[k], rc[k]), (name, k)


@pytest.mark.parametrize("name", ["mixed", "fb_strided_rows", "skip_touching"])
def test_fused_skip_if_raised(gpu_pkg, name):
    """A raised id flag: the fused kernel (and its fallback) changes nothing but g and the partials."""
    ops, lib = gpu_pkg.ops, gpu_pkg.lib
    spec = dict(next(s for s in FUSED if s["name"] == name), flags=True)
    w = _World(ops, lib, spec)
    try:
        _raise_flag(ops)
        w.run_fused()
        w.check_after(updated=False)
    finally:
        _clear_flags(ops)
    _check_pair(ops, lib, spec)               # flags clear: the normal update, pointer still passed


def _small_segs(k):
    return [(16 * i, 1, 8, 8, (2, 17, 40)[i % 3], SHIFT * (i % 2), (3, 1)[i % 2]) for i in range(k)]


@pytest.mark.parametrize("extra", [12, 13])
def test_fold_plan_merge(gpu_pkg, extra):
    """20 + 12 segments fit (all 32 in dst); 20 + 13 do not: src is folded into g at once, dst
    keeps its 20, and the fused update still equals fold-then-update and the fp64 reference."""
    ops, lib = gpu_pkg.ops, gpu_pkg.lib
    spec = dict(name=f"merge{extra}", n=N4, segs=_small_segs(20 + extra))
    b = _World(ops, lib, spec).run_separate()
    c = _World(ops, lib, spec)
    dst = _plan(lib, c.descs(range(20)))
    src = _plan(lib, c.descs(range(20, 20 + extra)))
    assert (dst.n, src.n) == (20, extra)
    lib.call("ttmi_fold_plan_merge", ctypes.byref(dst), ctypes.byref(src), _stream())
    assert dst.n == (32 if extra == 12 else 20)
    if extra == 13:                           # folded already: their partials consumed, g holds the sums
        g32, _ = c.expected_gradient()
        got = _np(c.st.g)
        for i in range(20, 33):
            c.folds[i].check_parts()
            assert _same(got[16 * i:16 * i + 8], g32[16 * i:16 * i + 8])
        assert _same(got[:320], c.g0[:320])
    c.fused(dst)
    rb, rc = b.check_after(), c.check_after()
    for k in rb:
        assert _same(rb[k], rc[k]), k


def test_fold_plan_run(gpu_pkg):
    """ttmi_fold_plan_run on a plan: the bits of ttmi_wgrad_fold on the same descriptors."""
    ops, lib = gpu_pkg.ops, gpu_pkg.lib
    spec = next(s for s in FUSED if s["name"] == "mixed")
    a, b = _World(ops, lib, spec), _World(ops, lib, spec)
    _run_folds(lib, a.descs())
    plan = _plan(lib, b.descs())
    assert plan.n == len(spec["segs"])
    assert _same(_np(b.st.g), b.g0)           # planning folds nothing
    lib.call("ttmi_fold_plan_run", ctypes.byref(plan), _stream())
    assert _same(_np(a.st.g), _np(b.st.g))
    assert _same(_np(a.st.g), a.expected_gradient()[0])
    for f in a.folds + b.folds:
        f.check_parts()


def test_fused_bias_rows(gpu_pkg):
    """A real weight gradient with a bias through deferred_wgrad(defer_fold=True): the plan's
    segment carries the bias row sums (store1 / part_rs).  Integer-valued bf16 operands, so the
    GEMM is exact and the float64 gradient is the fp32 one."""
    ops, lib = gpu_pkg.ops, gpu_pkg.lib
    M = N = 128
    R = next(r for r in range(8, 4096, 8) if lib.load().ttmi_wgrad_workspace(r, M, N, M, N) > 0)
    n, ow, ob = 20480, 1024, 1024 + M * N + 64
    hyper, t = HYPERS[0], 3
    rng = np.random.default_rng(12)
    before = _rand_state(rng, n)
    g0 = rng.standard_normal(n).astype(F32)
    g0[ow:ow + M * N] = rng.integers(-8, 9, size=M * N)
    g0[ob:ob + M] = rng.integers(-8, 9, size=M)
    dy = rng.integers(-2, 3, size=(R, M)).astype(F32)
    x = rng.integers(-2, 3, size=(R, N)).astype(F32)
    g32 = g0.astype(np.float64)
    g32[ow:ow + M * N] += (dy.astype(np.float64).T @ x.astype(np.float64)).reshape(-1)
    g32[ob:ob + M] += dy.astype(np.float64).sum(axis=0)
    assert _same(g32.astype(F32).astype(np.float64), g32)
    g32 = g32.astype(F32)
    dyd, xd = _dev(dy).to(torch.bfloat16), _dev(x).to(torch.bfloat16)
    res = []
    for fold_in_update in (False, True):
        st = _State(before[0], g0, before[1], before[2], hyper, t)
        gw, gb = st.g[ow:ow + M * N].view(M, N), st.g[ob:ob + M]
        with ops.deferred_wgrad(defer_fold=fold_in_update) as pend:
            ops.linear_dw(dyd, xd, gw, gb)
        if fold_in_update:
            assert pend.plan is not None and pend.plan.n == 1
            assert _same(_np(st.g), g0)       # nothing folded yet
        ops.adamw(st.p, st.g, st.m, st.v, st.mirror, st.hyper, st.step, zero_grad=True,
                  fold_plan=pend.plan if fold_in_update else None)
        torch.cuda.synchronize()
        del pend                              # the partials were kept alive until the update was issued
        assert not _np(st.g).any() and st.mirror_ok()
        _assert_step_close(f"bias_rows fused={fold_in_update}", before, g32, st.pmv(), hyper, t)
        res.append(st.pmv() + (_bits16(st.mirror),))
    for a, b in zip(*res):
        assert _same(a, b)


def test_fused_graph_replay(gpu_pkg):
    """One fused case captured with the step increment inside the graph and replayed twice: the
    bits of two eager steps (the second sees the consumed partials and the cleared g)."""
    ops, lib = gpu_pkg.ops, gpu_pkg.lib
    spec = next(s for s in FUSED if s["name"] == "mixed")
    eager, cap = _World(ops, lib, spec), _World(ops, lib, spec)
    plan_e = _plan(lib, eager.descs())
    for _ in range(2):
        ops.step_inc(eager.st.step)
        eager.fused(plan_e)
    plan_c = _plan(lib, cap.descs())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ops.step_inc(cap.st.step)
            cap.fused(plan_c)
    torch.cuda.current_stream().wait_stream(s)
    assert _same(cap.st.pmv()[0], cap.before[0])      # captured, not run
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert int(cap.st.step) == int(eager.st.step) == cap.t + 2
    re, rc = eager.result(), cap.result()
    for k in re:
        assert _same(re[k], rc[k]), k
    assert not _same(re["p"], eager.before[0]) and not _np(cap.st.g).any()
