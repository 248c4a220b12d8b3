"""CPU-side checks of the native boundary: the C-ABI library loads and exports every symbol include/vqk.h
declares (no compute calls without a GPU), and the product package never imports the oracle."""
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'vqvae-vqgan-pytorch-lightning_amd'


def header_symbols():
    text = open(os.path.join(ROOT, 'include', 'vqk.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(vqk_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_declared_symbol():
    native = importlib.import_module(PKG + '._native')
    native.build()
    lib = native.lib()
    syms = header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), s
    assert sorted(native.EXPORTS) == syms                  # ctypes prototypes cover the whole header
    assert lib.vqk_arch() == b'gfx950'
    assert lib.vqk_status_str(0) == b'ok' and lib.vqk_status_str(-1) != b'ok'


def test_argument_validation_without_gpu():
    """shape / pointer validation happens before any launch, so it is testable on the CPU box"""
    lib = importlib.import_module(PKG + '._native').lib()
    assert lib.vqk_vq_assign_f32(0, 0, 0, 0, 16, 8, 16, 0, 0, 0) == -5           # NULL pointers
    assert lib.vqk_conv2d_fprop(0, 16, 16, 0, 0, 16, 0, 1, 4, 4, 3, 8, 3, 0, 0, 0, 16, 0) == -1   # Cin % 4
    assert lib.vqk_conv2d_fprop(7, 16, 16, 0, 0, 16, 0, 1, 4, 4, 4, 8, 3, 0, 0, 0, 16, 0) == -2   # dtype
    assert lib.vqk_gn_stats(0, 16, 1, 16, 30, 32, 1e-6, 16, 16, 0) == -1                          # C % groups


def test_stride2_entry_points_validate_without_gpu():
    """round 4: the discriminator's stride-2 conv / data gradient (vqk_conv2d_s2_*) and the fused blur-adjoint + activation
    gradient refuse unsupported shapes and NULL pointers before any launch"""
    lib = importlib.import_module(PKG + '._native').lib()
    assert lib.vqk_conv2d_s2_supported(1, 16, 128, 128, 128, 256, 0) == 1 and lib.vqk_conv2d_s2_supported(1, 16, 128, 128, 128, 256, 1) == 1
    assert lib.vqk_conv2d_s2_supported(1, 16, 8, 8, 512, 512, 0) == 0            # 17x17 -> 8x8 stays on the im2col kernel
    assert lib.vqk_conv2d_s2_supported(0, 16, 128, 128, 128, 256, 0) == 0        # fp32
    assert lib.vqk_conv2d_s2_supported(1, 64, 128, 128, 512, 256, 0) == 0        # 32-bit buffer offsets
    assert lib.vqk_conv2d_s2_fprop(1, 0, 0, 0, 0, 16, 128, 128, 128, 256, 3, 1.0, 1.0, 0, 0) == -5
    assert lib.vqk_conv2d_s2_dgrad(1, 0, 0, 0, 0, 16, 128, 128, 128, 256, 1.0, 0, 0) == -5
    assert lib.vqk_upfirdn2d_act_backward(1, 0, 0, 0, 0, 2, 33, 33, 64, 1, 1, 1, 1, 1, 1.0, 3, 32, 32, 0) == -5
    assert lib.vqk_conv_packed_elems(256, 128, 3, 3) == 256 * 128 * 9            # layout 3: the nine taps, grouped by parity


def test_pack_weights_validates_without_gpu():
    """vqk_conv_pack_weights refuses before any launch: NULL pointers and unknown layouts, tap counts other than 1x1 / 3x3, input
    channels that are no whole chunks, unknown dtypes, and -- the fragment-major layouts move 16-byte pieces -- misaligned buffers"""
    lib = importlib.import_module(PKG + '._native').lib()
    w, out = 0x10000, 0x20000                                                    # never dereferenced: every call below is refused
    assert lib.vqk_conv_pack_weights(0, out, 1, 128, 64, 3, 0, 1, 0) == -5       # VQK_ERR_ARG
    assert lib.vqk_conv_pack_weights(w, 0, 1, 128, 64, 3, 0, 1, 0) == -5
    assert lib.vqk_conv_pack_weights(w, out, 1, 128, 64, 3, 0, 4, 0) == -5       # no layout 4
    assert lib.vqk_conv_pack_weights(w, out, 1, 128, 64, 2, 0, 1, 0) == -1       # VQK_ERR_SHAPE: ksize 2
    assert lib.vqk_conv_pack_weights(w, out, 1, 128, 32, 3, 0, 1, 0) == -1       # bf16 chunks are 64 channels
    assert lib.vqk_conv_pack_weights(w, out, 1, 32, 128, 3, 1, 1, 0) == -1       # (transposed: the chunks are of Cout)
    assert lib.vqk_conv_pack_weights(w, out, 0, 128, 32, 3, 0, 2, 0) == -1       # the phase operand is bf16, its split form fp32
    assert lib.vqk_conv_pack_weights(w, out, 1, 128, 64, 3, 0, 6, 0) == -1
    assert lib.vqk_conv_pack_weights(w, out, 1, 128, 64, 3, 0, 3, 0) == -1       # layout 3 is a data-gradient operand
    assert lib.vqk_conv_pack_weights(w, out, 7, 128, 64, 3, 0, 1, 0) == -2       # VQK_ERR_DTYPE
    assert lib.vqk_conv_pack_weights(w + 4, out, 1, 128, 64, 3, 0, 1, 0) == -3   # VQK_ERR_ALIGN
    assert lib.vqk_conv_pack_weights(w, out + 8, 0, 128, 32, 3, 0, 5, 0) == -3


def test_ops_refuse_cpu_tensors():
    import torch
    ops = importlib.import_module(PKG + '.ops')
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.conv2d(torch.zeros(1, 4, 4, 4), torch.zeros(4, 4, 3, 3))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.vq_assign(torch.zeros(8, 8), torch.zeros(4, 8), 0)


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, PKG)):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle', src, flags=re.M), f


def test_tuning_slots_replace_environment_reads():
    """VERDICT r3 hygiene: the library reads no environment variable; its launch heuristics are named tuning slots
    (include/vqk.h: vqk_set_tuning), unknown names are refused, and the Python loader maps VQK_<SLOT> variables onto them"""
    native = importlib.import_module(PKG + '._native')
    lib = native.lib()
    names = [lib.vqk_tuning_name(i).decode() for i in range(lib.vqk_tuning_count())]
    assert 'MX_HALF' in names and 'GN_BLOCKS_REDUCE' in names and len(names) == len(set(names)) >= 20
    assert lib.vqk_set_tuning(b'NO_SUCH_SLOT', 1) == -5
    assert lib.vqk_set_tuning(b'MX_HALF', 0) == 0 and lib.vqk_reset_tuning() == 0
    got = native.apply_env_tuning(lib, {'VQK_MX_HALF': '0', 'VQK_WGMX_COEF': '0.16', 'VQK_GN_NO_SMALL': '1', 'VQK_UNRELATED': '7'})
    assert got == {'MX_HALF': 0, 'WGMX_COEF_E4': 1600, 'GN_NO_SMALL': 1}
    assert lib.vqk_reset_tuning() == 0
    import glob
    import os
    csrc = os.path.join(os.path.dirname(native.__file__), 'csrc')
    for path in glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.cpp')) + glob.glob(os.path.join(csrc, '*.h')):
        assert 'getenv' not in open(path).read(), path
