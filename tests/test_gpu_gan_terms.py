"""The GAN loss-term kernels (csrc/disc.hip: one reduce and one gradient kernel behind vo_gan_reduce / _grad and
their _multi forms) against arithmetic done elsewhere, through tests/gan_check.py: float64 sums with the derived
bar, gradients bit for bit against the fp32 expression on the CPU, guards, NaN padding, determinism.  The cases are
the smallest at which each piece can go wrong; tests/test_gan_check.py checks the checker on them without a GPU.
The leaky-ReLU mask at the widths test_gpu_gan.py leaves out.
"""

import ctypes

import pytest
import torch

import gan_check as GC
from gan_check import case, term


def _cases(dt):
    c = [
        # widths and layouts (rows x width, lda): one vector; scalar strided; vector strided; flat; base offset by
        # 4 elements (bf16: 8 bytes, the scalar path; fp32: 16 bytes, still vectors); b strided, a contiguous
        case("w8_one_vector", dt, [term(0, 1, 8, special=False)]),
        case("w11_lda13", dt, [term(1, 5, 11, lda=13, scale=-0.5)]),
        case("w64_lda72", dt, [term(0, 5, 64, lda=72, ldb=80, scale=0.25, special=True)]),
        case("w64_flat", dt, [term(2, 5, 64, special=True)]),
        case("w64_off4", dt, [term(1, 5, 64, off=4, special=True)]),
        case("w64_b_strided", dt, [term(0, 5, 64, ldb=72, scale=-2.0)]),
        # units per path: 1, around one block, past the reduction's 512-block cap (a second trip per thread)
        case("scalar_u1", dt, [term(2, 1, 1)]),
        case("scalar_u255", dt, [term(0, 1, 255, special=True)]),
        case("scalar_u256", dt, [term(1, 4, 64, lda=68)]),
        case("scalar_u257", dt, [term(2, 1, 257, scale=-1.0)]),
        case("vector_u255", dt, [term(1, 1, 2040)]),
        case("vector_u256", dt, [term(2, 1, 2048)]),
        case("vector_u257", dt, [term(0, 1, 2056, scale=3.0)]),
        case("scalar_u512x256+1", dt, [term(2, 1, 512 * 256 + 1)]),
        case("vector_u512x256+1", dt, [term(1, 1, (512 * 256 + 1) * 8, scale=-1.0)]),
        # past the gradient's 4096-block cap
        case("scalar_u4096x256+1", dt, [term(1, 1, 4096 * 256 + 1, scale=0.5)], grad_cap=True),
        case("vector_u4096x256+1", dt, [term(2, 1, (4096 * 256 + 1) * 8)], grad_cap=True),
    ]
    # term tables: 32 (one full table) and 33 (split), vector and scalar terms mixed, every kind next to the others
    mixed = lambda n: [term(j % 3, 3, 16, lda=24, ldb=16, scale=(-1) ** j * (1 + j / 8), special=j < 3) if j % 2 == 0
                       else term((j // 2) % 3, 3, 11, lda=13, ldb=11, scale=0.5 + j / 16, special=j < 6)
                       for j in range(n)]
    return c + [case("terms32", dt, mixed(32)), case("terms33", dt, mixed(33))]


CASES = _cases("bf16") + _cases("f32")


class _Ops:
    """ops' four entry points, and the multi reduction on the caller's output vector and workspace."""

    def __init__(self):
        from visual_onoma_to_wave_amd import ops
        self.ops = ops
        self.gan_reduce, self.gan_reduce_grad = ops.gan_reduce, ops.gan_reduce_grad
        self.gan_reduce_multi, self.gan_reduce_grad_multi = ops.gan_reduce_multi, ops.gan_reduce_grad_multi

    def gan_reduce_multi_into(self, kinds, As, Bs, scale, out, ws):
        from visual_onoma_to_wave_amd import _lib
        ops = self.ops
        arr, keep = ops._gan_terms(kinds, As, Bs)
        _lib.check(_lib.lib().vo_gan_reduce_multi(len(kinds), ctypes.cast(arr, ctypes.c_void_p), ops.vo_dtype(As[0]),
                                                  scale.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                  ops._stream(As[0])), "vo_gan_reduce_multi")
        del keep


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_gan_terms_against_float64_and_fp32_expression(c):
    m = GC.make(c)
    ref = GC.reference(c, m)
    GC.run(c, m, _Ops(), "cuda")
    GC.verify(c, m, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("gdt,rdt", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                     (torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)])
@pytest.mark.parametrize("width,ld,off", [(8, 8, 0), (11, 13, 0), (64, 64, 4)])
def test_lrelu_mask_widths_exact(gdt, rdt, width, ld, off):
    """vo_lrelu_mask at one vector per row, at a scalar strided width and at a base offset by 4 elements (the
    scalar kernel where that is not 16 bytes), exact against torch on the CPU: the mask is one multiply.  The
    padding columns of ref hold NaN."""
    from visual_onoma_to_wave_amd import ops
    rows, slope = 37, 0.1
    gen = torch.Generator().manual_seed(width * 100 + off)
    g = torch.randn(off + rows * width, generator=gen).to(gdt)
    rbuf = torch.full((off + rows * ld,), float("nan")).to(rdt)
    gv = g.as_strided((rows, width), (width, 1), off)
    rv = rbuf.as_strided((rows, width), (ld, 1), off)
    rv.copy_(torch.randn(rows, width, generator=gen))
    want = (gv.float() * torch.where(rv.float() > 0, 1.0, slope)).to(gdt)
    gd, rd = g.cuda(), rbuf.cuda()
    got = ops.lrelu_mask(gd.as_strided((rows, width), (width, 1), off), rd.as_strided((rows, width), (ld, 1), off),
                         slope)
    assert torch.equal(got.cpu().view(torch.int16 if gdt == torch.bfloat16 else torch.int32),
                       want.view(torch.int16 if gdt == torch.bfloat16 else torch.int32))
