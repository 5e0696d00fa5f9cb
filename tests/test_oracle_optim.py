"""The CPU optimizer reference (oracle/optim_ref.py) against torch itself: adamw_step64 is
torch.optim.AdamW on float64 CPU tensors to 1e-12 relative, over 3 steps with the learning rate
changed between steps; the two fold restatements agree with each other where both are exact."""
import numpy as np
import pytest
import torch

from oracle import optim_ref as oref


@pytest.mark.parametrize("hyper", oref.HYPERS)
def test_adamw_step64_is_torch_adamw_float64(hyper):
    lr, b1, b2, eps, wd = hyper
    gen = torch.Generator().manual_seed(5)
    n = 1001
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    w = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([w], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    pn, mn, vn = p.numpy().copy(), np.zeros(n), np.zeros(n)      # torch starts its moments at zero
    for t in range(1, 4):
        g = torch.randn(n, generator=gen, dtype=torch.float64)
        g[::7] = 0.0
        lr_t = lr * (1.0 + 0.5 * (t - 1))                        # a schedule: lr changes every step
        opt.param_groups[0]["lr"] = lr_t
        w.grad = g.clone()
        opt.step()
        pn, mn, vn = oref.adamw_step64(pn, g.numpy(), mn, vn, (lr_t, b1, b2, eps, wd), t)
        st = opt.state[w]
        for name, got, want in (("p", pn, w.detach().numpy()), ("m", mn, st["exp_avg"].numpy()),
                                ("v", vn, st["exp_avg_sq"].numpy())):
            err = np.abs(got - want).max() / np.abs(want).max()
            assert err <= 1e-12, (name, t, err)


def test_adamw_step64_leaves_its_inputs():
    p = np.ones(4, dtype=np.float32)
    g = np.full(4, 0.5, dtype=np.float32)
    m = np.zeros(4, dtype=np.float32)
    v = np.zeros(4, dtype=np.float32)
    out = oref.adamw_step64(p, g, m, v, oref.HYPERS[0], 1)
    assert all(o.dtype == np.float64 for o in out)
    assert (p == 1).all() and (m == 0).all() and (v == 0).all()
    # t = 1 from zero moments: m_hat = g, v_hat = g², the step is lr·g/(|g| + eps) after the decay
    lr, _, _, eps, wd = oref.HYPERS[0]
    assert np.allclose(out[0], 1.0 * (1 - lr * wd) - lr * 0.5 / (0.5 + eps), rtol=1e-13, atol=0)


@pytest.mark.parametrize("S,s_stride,M,N", [(1, 8, 1, 8), (5, 24, 2, 8), (17, 16, 2, 8)])
def test_folds_agree_on_exactly_representable_partials(S, s_stride, M, N):
    rng = np.random.default_rng(S)
    n = (S - 1) * s_stride + M * N
    c = rng.integers(-8, 9, size=(M, N)).astype(np.float32)
    part = rng.integers(-64, 65, size=n).astype(np.float32)       # small integers: every sum is exact
    for acc in (0, 1, 2, 3):
        a = oref.fold64(part, S, s_stride, M, N, c, acc, 0)
        b = oref.fold32_in_order(part, S, s_stride, M, N, c, acc, 0)
        assert a.dtype == np.float64 and b.dtype == np.float32
        assert np.array_equal(a, b.astype(np.float64))
        want = sum(part[s * s_stride: s * s_stride + M * N].reshape(M, N).astype(np.float64) for s in range(S))
        assert np.array_equal(a, want + (c if acc & 1 else 0))
    q = rng.integers(-(1 << 40), 1 << 40, size=n, dtype=np.int64)
    a = oref.fold64(q, S, s_stride, M, N, c, 1, 36)
    b = oref.fold32_in_order(q, S, s_stride, M, N, c, 1, 36)
    tot = sum(int(q[s * s_stride]) for s in range(S))             # python integers: exact
    assert a[0, 0] == float(c[0, 0]) + tot / 2.0 ** 36
    assert b[0, 0] == np.float32(c[0, 0] + np.float32(tot / 2.0 ** 36))
    assert np.abs(a - b).max() <= 2.0 ** -23 * np.abs(a).max()


def test_fold_rejects_short_partials():
    with pytest.raises(ValueError):
        oref.fold64(np.zeros(10, dtype=np.float32), 2, 8, 1, 8, None, 0, 0)
    with pytest.raises(TypeError):
        oref.fold64(np.zeros(16, dtype=np.float32), 2, 8, 1, 8, None, 0, 36)
