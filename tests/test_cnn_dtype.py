"""CPU checks of the item encoders' storage-mode keyword (cnn.py ``dtype``, the models'
``encoder_dtype``): only bf16 / fp32 are accepted, the parameters do not depend on the mode, and
the default stays bf16."""
import inspect

import pytest
import torch


def test_unsupported_dtype_raises_at_construction(pkg):
    with pytest.raises(TypeError, match="bfloat16 or torch.float32"):
        pkg.cnn.ResNet18(1, 128, dtype=torch.float16)
    with pytest.raises(TypeError, match="bfloat16 or torch.float32"):
        pkg.cnn.TabularEncoder(8, 128, dtype=torch.float64)
    with pytest.raises(TypeError):
        pkg.cnn.AudioEncoder(128, dtype=torch.float16)
    with pytest.raises(TypeError):
        pkg.cnn.VisualEncoder(128, dtype=torch.int8)


def test_state_dict_does_not_depend_on_the_mode(pkg):
    a = pkg.cnn.ResNet18(3, 64).state_dict()
    b = pkg.cnn.ResNet18(3, 64, dtype=torch.float32).state_dict()
    assert list(a.keys()) == list(b.keys())
    assert all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
    ta = pkg.cnn.TabularEncoder(37, 128).state_dict()
    tb = pkg.cnn.TabularEncoder(37, 128, dtype=torch.float32).state_dict()
    assert list(ta.keys()) == list(tb.keys())
    # checkpoints interchange
    pkg.cnn.ResNet18(3, 64, dtype=torch.float32).load_state_dict(a)


def _model(pkg, **kw):
    return pkg.TwoTowerModel(vocab_size=50, tabular_input_dim=8, num_genders=2, num_countries=3,
                             max_seq_len=8, user_embedding_dim=128, item_embedding_dim=128,
                             precomputed_modalities=False, with_text=False, **kw)


def test_two_tower_encoder_dtype_keyword(pkg):
    sig = inspect.signature(pkg.TwoTowerModel.__init__)
    assert sig.parameters["encoder_dtype"].default == torch.bfloat16
    assert inspect.signature(pkg.item_tower.MultimodalItemEncoder.__init__) \
        .parameters["encoder_dtype"].default == torch.bfloat16
    m = _model(pkg)
    it = m.item_tower
    assert it.encoder_dtype == torch.bfloat16
    assert it.audio_encoder.backbone.dtype == it.visual_encoder.backbone.dtype == torch.bfloat16
    assert it.tabular_encoder.dtype == torch.bfloat16
    # compute_dtype alone does not move the encoders (it keeps its meaning)
    m32 = _model(pkg, compute_dtype=torch.float32)
    assert m32.item_tower.audio_encoder.backbone.dtype == torch.bfloat16
    assert m32.item_tower.compute_dtype == torch.float32
    f = _model(pkg, encoder_dtype=torch.float32)
    it = f.item_tower
    assert it.audio_encoder.backbone.dtype == it.visual_encoder.backbone.dtype == torch.float32
    assert it.tabular_encoder.dtype == torch.float32
    assert it.compute_dtype == torch.bfloat16
    assert list(f.state_dict().keys()) == list(m.state_dict().keys())
    with pytest.raises(TypeError):
        _model(pkg, encoder_dtype=torch.float16)


def test_fp32_descriptor_the_kernels_do_not_serve_is_refused(pkg):
    """The space-to-depth stem modes and the DGRAD-fused BatchNorm reduction exist in bf16
    storage only: an fp32 descriptor asking for them fails in the plan (no launch), with a
    message; the plain modes plan as in bf16."""
    import ctypes
    L = pkg.lib
    lib = L.load()

    def desc(mode, **kw):
        d = L.ConvDesc()
        d.mode, d.N, d.H, d.W, d.C, d.Cin, d.Co = mode, 2, 16, 16, 64, 64, 64
        d.KH = d.KW = 3
        d.stride, d.pad = 1, 1
        d.f32 = 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert lib.ttmi_conv2d_workspace(ctypes.byref(desc(2))) > 0
    assert lib.ttmi_conv2d_workspace(ctypes.byref(desc(1))) == 0
    stem = dict(C=8, Cin=1, KH=7, KW=7, stride=2, pad=3)
    for mode in (3, 4):
        assert lib.ttmi_conv2d_workspace(ctypes.byref(desc(mode, **stem))) == -1
        assert b"no fp32-storage kernel" in lib.ttmi_last_error()
        with pytest.raises(L.TTMIError, match="no fp32-storage kernel"):
            L.call("ttmi_conv2d", ctypes.byref(desc(mode, **stem)), None)
    with pytest.raises(L.TTMIError, match="bn_sums"):
        L.call("ttmi_conv2d", ctypes.byref(desc(1, bn_sums=256, bn_x=256, bn_mean=256, bn_rstd=256)), None)
    with pytest.raises(L.TTMIError, match="f32 must be 0"):
        L.call("ttmi_conv2d", ctypes.byref(desc(0, f32=2)), None)


def test_mixed_storage_dtypes_raise(pkg):
    """The conv / BatchNorm2d / pool wrappers dispatch on the tensors' dtype and refuse a mix
    before any library call."""
    ops = pkg.ops
    xb = torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16)
    xf = torch.zeros(1, 4, 4, 8)
    idx = torch.zeros(1, 2, 2, 8, dtype=torch.uint8)
    with pytest.raises(TypeError, match="all bf16 or all fp32"):
        ops.maxpool_fwd(xb, 3, 2, 1, torch.zeros(1, 2, 2, 8), idx)
    with pytest.raises(TypeError, match="all bf16 or all fp32"):
        ops.bn2d_fwd(xf, None, None, torch.ones(8), torch.zeros(8), torch.zeros_like(xb),
                     torch.zeros(8), torch.zeros(8), running_mean=torch.zeros(8), running_var=torch.ones(8))
    with pytest.raises(TypeError, match="all bf16 or all fp32"):
        ops.conv2d(ops.FWD, 1, 4, 4, 8, 8, 8, 3, 1, 1, x=xf, w=torch.zeros(8, 3, 3, 8, dtype=torch.bfloat16),
                   out=torch.zeros(1, 4, 4, 8))
    with pytest.raises(TypeError, match="all bf16 or all fp32"):
        ops.avgpool_fwd(xf, torch.zeros(1, 8, dtype=torch.float16))
