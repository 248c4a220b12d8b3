"""Bias gradients that ride in a kernel which streams (or writes) the gradient tensor anyway, against the column-sum pass they
replace (raw_colsum on the same tensor):

* the decoder head's conv (128 -> 3 of 8 padded channels): the edge weight-gradient launch gathers the sums of dy from its own
  staged copy (vqk_conv2d_wgrad_edge_bias); dW is bit-identical to the launch without the extra output;
* the decoder's last Upsample conv, whose output is read by the decoder's final norm: that norm's backward carries the sums
  (GroupNormSiLUFn, sole_consumer; the kernel is vqk_gn_backward_colsum's, tested in tests/test_gpu_gn_forms.py) -- checked on a
  small model, together with the launches that disappear.

The bound for the sums is the one the GroupNorm column-sum test uses (tests/test_gpu_gn_forms.py: _BOUNDS[...]['colsum'] = 5e-6,
relative 2-norm): both sides add the same bf16 values in fp32, in a different order.

NOT built: the sums in the single-kernel GroupNorm backwards of the maps of <= 1024 pixels.  The one-block-per-slice form's
column-sum passes take < 10 us each in the headline step (512 ch @16^2: 9.99 us, 256 ch @16^2: 8.9 us).  The cluster form
(256 ch @32^2: 21.6 us) was built and measured: with the extra accumulation the kernel compiles differently (168 against
204 VGPRs), its dx moves in last bits against the kernel without it, and bench.py --dump-outputs (AdamW with beta1 = 0 turns a sign
flip of a near-zero gradient into a full step) then differs from the previous build's by 1.8 where two runs of one build differ by 5e-5 (profiles/gn_pooled_skip_ab.txt).
"""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

PKG = 'vqvae-vqgan-pytorch-lightning_amd'
ops = importlib.import_module(PKG + '.ops')
native = importlib.import_module(PKG + '._native')
DEV, F32, BF, CL = 'cuda:0', torch.float32, torch.bfloat16, torch.channels_last
COLSUM_BOUND = 5e-6                               # tests/test_gpu_gn_forms.py: _BOUNDS[dtype]['colsum']
EPS = 1e-6


def _relnorm(a, r):
    return float((a.double() - r.double()).norm() / (r.double().norm() + 1e-300))


# ------------------------------------------------------------------------------------------ the decoder head's conv
def _edge(x, dy, dw, db):
    n, cin, h, w = x.shape
    ws = ops._edge_ws(x.device)
    st = native.lib().vqk_conv2d_wgrad_edge_bias(ops.dcode(BF), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ops._p(db), ws.data_ptr(),
                                                 ws.numel() * 4, n, h, w, cin, dy.shape[1], 3, ops.zero_page(x.device).data_ptr(),
                                                 ops._stream())
    native.check(st, 'conv2d_wgrad_edge_bias')
    torch.cuda.synchronize()


@pytest.mark.parametrize('n,c,h,w', [(2, 8, 16, 32), (1, 8, 8, 16)])
def test_head_conv_bias_rides_in_the_edge_weight_gradient(n, c, h, w):
    g = torch.Generator(device=DEV).manual_seed(h * w + n)
    x = torch.randn(n, 128, h, w, device=DEV, generator=g).to(BF).contiguous(memory_format=CL)
    dy = (torch.randn(n, c, h, w, device=DEV, generator=g) + 0.25).to(BF).contiguous(memory_format=CL)    # (pad channels non-zero: they must be dropped)
    dw0 = torch.randn(3 * 9 * 128, device=DEV, generator=g)
    db0 = torch.randn(3 + 5, device=DEV, generator=g)                  # 3 true channels + a guard behind them
    dw_plain, dw_fold, db = dw0.clone(), dw0.clone(), db0.clone()
    _edge(x, dy, dw_plain, None)
    _edge(x, dy, dw_fold, db)
    assert torch.equal(dw_fold, dw_plain)                              # the host kernel's own output: bit-identical
    assert not torch.equal(dw_plain, dw0)
    assert torch.equal(db[3:], db0[3:])                                # nothing written past the true channels
    ref = ops.raw_colsum(n * h * w, c, dy)[:3]
    got = db[:3].double() - db0[:3].double()
    assert _relnorm(got, ref) < COLSUM_BOUND, (_relnorm(got, ref), got, ref)
    exact = dy.double().sum((0, 2, 3))[:3]
    assert _relnorm(got, exact) < COLSUM_BOUND


def test_head_conv_bias_is_refused_on_the_first_conv_and_in_deterministic_mode():
    x = torch.zeros(1, 8, 8, 16, device=DEV, dtype=BF).contiguous(memory_format=CL)
    dy = torch.zeros(1, 128, 8, 16, device=DEV, dtype=BF).contiguous(memory_format=CL)
    dw, db, ws = torch.zeros(128 * 9 * 3, device=DEV), torch.zeros(8, device=DEV), ops._edge_ws(torch.device(DEV))
    st = native.lib().vqk_conv2d_wgrad_edge_bias(ops.dcode(BF), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                                 ws.numel() * 4, 1, 8, 16, 8, 128, 3, ops.zero_page(x.device).data_ptr(), ops._stream())
    assert st == -5                                                    # VQK_ERR_ARG: thin x, wide dy -- no staged copy of dy's columns
    xl, dyl = dy, x                                                    # (128 -> 8: the last conv's shapes)
    ops.set_deterministic(True)
    try:
        assert not ops.edge_wgrad_takes_bias(xl, dyl, 3, False)        # ordered mode keeps the standalone ordered sum
    finally:
        ops.set_deterministic(False)
    assert ops.edge_wgrad_takes_bias(xl, dyl, 3, False)


# ------------------------------------------------------------------------------------------ small maps
def test_small_maps_keep_the_column_sum_pass():
    """(2, 256, 16, 16) and (2, 512, 32, 32): the single-kernel GroupNorm backwards of maps of <= 1024 pixels carry no sums (module
    docstring), so the host must not hand them a bias to sum -- that would route them onto the slower two-kernel passes"""
    assert not ops.gn_colsum_ok(16, 16) and not ops.gn_colsum_ok(32, 32) and ops.gn_colsum_ok(32, 64)


# ------------------------------------------------------------------------------------------ the model's walk
def _model_grads(on):
    model_mod = importlib.import_module(PKG + '.model')
    trainer_mod = importlib.import_module(PKG + '.trainer')
    saved = ops.FUSE_BIAS_COLSUM
    ops.FUSE_BIAS_COLSUM = on
    try:
        torch.manual_seed(3)
        ae = dict(channels=128, num_res_blocks=1, channel_multipliers=(1, 2))
        qc = dict(num_embeddings=256, embedding_dim=256, reinit_every_n_epochs=None, type='standard', params=dict(commitment_cost=0.25))
        tc = dict(lr=1e-4, betas=(0.0, 0.99), eps=1e-8, weight_decay=1e-4, warmup_epochs=None, decay_epochs=None)
        m = model_mod.VQVAE(64, ae, qc, None, tc, compute_dtype=BF).to(DEV).train()
        tr = trainer_mod.MiniTrainer(num_training_batches=4)
        opt = tr.attach(m)[0]
        m.on_train_start()
        images = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
        calls = {}
        lib = native.lib()

        class Counting:
            def __getattr__(self, name):
                fn = getattr(lib, name)
                if name in ('vqk_colsum_lead', 'vqk_gn_backward_colsum', 'vqk_conv2d_wgrad_edge_bias'):
                    def wrapped(*a, _fn=fn, _n=name):
                        if _n != 'vqk_conv2d_wgrad_edge_bias' or a[4]:             # (the edge launch counts when it carries db)
                            calls[_n] = calls.get(_n, 0) + 1
                        return _fn(*a)
                    return wrapped
                return fn
        real = ops._native.lib
        ops._native.lib = lambda: Counting()
        try:
            opt.zero_grad()
            m.training_step(images, 0).backward()
        finally:
            ops._native.lib = real
        torch.cuda.synchronize()
        ops.check_kernel_health()
        return {k: p.grad.detach().float().clone() for k, p in m.named_parameters() if p.grad is not None}, calls
    finally:
        ops.FUSE_BIAS_COLSUM = saved


def test_model_bias_gradients_with_and_without_the_folds():
    g_sep, c_sep = _model_grads(False)
    g_fus, c_fus = _model_grads(True)
    assert c_sep.get('vqk_gn_backward_colsum', 0) == 0 and c_sep.get('vqk_conv2d_wgrad_edge_bias', 0) == 0
    assert c_fus.get('vqk_conv2d_wgrad_edge_bias', 0) == 1                          # the head conv
    assert c_fus.get('vqk_gn_backward_colsum', 0) >= 1                              # the last Upsample conv, in the final norm's backward
    folded = c_fus['vqk_gn_backward_colsum'] + 1
    assert c_fus.get('vqk_colsum_lead', 0) == c_sep['vqk_colsum_lead'] - folded     # exactly those column-sum passes are gone
    for k in g_sep:                                                                 # (tests/test_gpu_bias_fusion.py's tolerance for bf16)
        err = float((g_fus[k] - g_sep[k]).norm() / (g_sep[k].norm() + 1e-20))
        assert err < 2e-3, (k, err)
    for k in ('decoder.conv_out.bias',) + tuple(k for k in g_sep if k.startswith('decoder.blocks') and k.endswith('.conv.bias')):
        assert float(g_fus[k].abs().max()) > 0, k
