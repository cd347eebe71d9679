"""LayerNorm (csrc/layernorm.hip) and BatchNorm (csrc/batchnorm.hip) kernels element by element against float64
(tests/norm_check.py) at their reduction, dtype, lens and data edges.  Each case calls the C entry point with
pointers into guarded buffers, then once more through the ops wrapper, and the two results must agree bit for
bit.  CASES and REQUIRED are plain data (no GPU at import): tests/test_norm_check.py checks on the CPU that the
cases reach every shipped instantiation, that every BatchNorm case's declared route record is vo_bn_route's, and
that the checker rejects its named faults on this very matrix."""

import ctypes

import pytest
import torch

import norm_check as NC
from norm_check import bn_case, ln_case

# ---- rel-L2 the fp32 stand-in reaches on the ill-conditioned cases (offset, constant), measured by
# test_norm_check.py::test_standin_rel_l2_of_ill_conditioned_cases_is_as_recorded on the CPU; verify allows 4 x
STANDIN_REL_L2 = {
    "ln_fwd_bf16_bf16_bf16_D512_B5_T5_mixed_offset": {"y": 1.655e-03},
    "ln_fwd_bf16_bf16_bf16_D256_B1_T1_nores_constant": {"y": 1.739e-03},
    "ln_fwd_f32_f32_f32_D512_B5_T5_full_offset": {"y": 1.624e-05},
    "ln_fwd_f32_f32_f32_D256_B3_T7_nores_zero_first_constant": {"y": 6.779e-05},
    "ln_fwd_bf16_bf16_f32_D512_B1_T1_offset": {"y": 8.602e-06},
    "ln_fwd_bf16_bf16_f32_D256_B7_T11_nores_zero_mid_constant": {"y": 6.659e-08},
    "ln_fwd_f32_f32_bf16_D512_B3_T7_zero_first_offset": {"y": 1.659e-03},
    "ln_fwd_f32_f32_bf16_D256_B3_T7_nores_constant": {"y": 1.672e-03},
    "ln_dual_f32_f32_f32_D512_B7_T11_zero_mid_offset": {"y": 2.131e-05},
    "ln_dual_bf16_bf16_f32_D256_B3_T3_one_constant": {"y": 5.155e-08},
    "ln_dual_bf16_f32_f32_D512_B3_T7_offset": {"y": 1.472e-05},
    "ln_drop_bf16_f32_f32_D256_B5_T5_p0.5_y16_mixed_constant": {"y": 6.671e-08},
    "ln_drop_f32_f32_f32_D512_B3_T3_p0.5_y16_one_offset": {"y": 2.680e-05},
    "ln_drop_f32_f32_f32_D256_B5_T5_p0.0_full_constant": {"y": 8.082e-05},
    "ln_drop_bf16_bf16_bf16_D512_B5_T5_p0.0_mixed_offset": {"y": 1.650e-03},
    "ln_drop_bf16_f32_f32_D256_B1_T1_p0.1_constant": {"y": 4.887e-08},
    "ln_bwd_bf16_bf16_bf16_D512_B1_T1_offset": {"gh": 1.636e-03, "dgamma": 9.533e-08, "dbeta": 0.000e+00},
    "ln_bwd_bf16_bf16_f32_D512_B31_T31_constant": {"gh": 1.658e-03, "dgamma": 1.264e-07, "dbeta": 1.212e-07},
    "ln_bwd_f32_f32_f32_D256_B31_T31_full_offset": {"gh": 1.773e-06, "dgamma": 1.865e-05, "dbeta": 1.124e-07},
    "ln_bwd_f32_f32_bf16_D256_B7_T439_one_constant": {"gh": 6.484e-08, "dgamma": 4.237e-05, "dbeta": 0.000e+00},
    "ln_bwd_ex_bf16_f32_f32_D512_B5_T205_zero_mid_offset": {
        "gres": 1.243e-06, "gh": 1.658e-03,
        "dgamma": 1.897e-05, "dbeta": 1.079e-07},
    "ln_bwd_ex_bf16_f32_bf16_D256_B17_T241_zero_first_constant": {
        "gres": 7.049e-08, "gh": 1.663e-03,
        "dgamma": 7.651e-05, "dbeta": 4.189e-08},
    "ln_bwd_ex_bf16_f32_bf16_D256_B31_T31_gy2_full_offset": {
        "gres": 1.671e-06, "gh": 1.659e-03,
        "dgamma": 1.876e-05, "dbeta": 3.360e-08},
    "ln_bwd_drop_bf16_f32_f32_D512_B31_T31_p0.5_offset": {
        "gres": 1.060e-06, "gh": 1.660e-03,
        "dgamma": 1.645e-05, "dbeta": 1.254e-07},
    "ln_bwd_drop_bf16_f32_bf16_D512_B3_T7_p0.1_mixed_constant": {
        "gres": 7.206e-08, "gh": 1.666e-03,
        "dgamma": 4.748e-07, "dbeta": 0.000e+00},
    "ln_bwd_drop_f32_f32_f32_D512_B7_T439_p0.5_one_constant": {
        "gres": 6.706e-08, "gh": 6.813e-08,
        "dgamma": 3.309e-07, "dbeta": 4.724e-08},
    "ln_bwd_drop_bf16_bf16_bf16_D512_B1_T1_p0.5_offset": {
        "gres": 1.647e-03, "gh": 1.619e-03,
        "dgamma": 1.041e-07, "dbeta": 0.000e+00},
    "bn_f32_f32_M511_C12_offset": {"y": 4.471e-05, "dgamma": 1.809e-07, "dbeta": 1.126e-07, "dx": 4.869e-08},
    "bn_f32_f32_M85_C80_constant": {"y": 6.890e-08, "dgamma": 1.212e-07, "dbeta": 9.147e-08, "dx": 3.486e-08},
    "bn_f32_f32_M97_C80_offset": {"y": 6.100e-05, "dgamma": 9.452e-08, "dbeta": 8.492e-08, "dx": 5.339e-08},
    "bn_bf16_bf16_M776_C80_offset": {"y": 1.694e-03, "dgamma": 1.285e-07, "dbeta": 1.747e-08, "dx": 1.654e-03},
    "bn_bf16_bf16_M509_C512_constant": {"y": 1.661e-03, "dgamma": 1.216e-07, "dbeta": 1.288e-08, "dx": 1.649e-03},
    "bn_f32_f32_M129_C1024_offset": {"y": 6.775e-05, "dgamma": 1.063e-07, "dbeta": 1.005e-07, "dx": 5.260e-08},
    "bn_f32_f32_M1028_C1_offset": {"y": 1.052e-05, "dx": 2.440e-08, "dgamma": 2.160e-08, "dbeta": 8.303e-09},
    "bn_f32_f32_M37_C65_offset": {"y": 6.967e-05, "dgamma": 8.378e-08, "dbeta": 7.579e-08, "dx": 5.074e-08},
    "bn_f32_f32_M37_C65_constant": {"y": 7.012e-08, "dgamma": 8.265e-08, "dbeta": 6.566e-08, "dx": 5.914e-08},
}

# ---- the vo_bn_route records (NC.BN_FIELDS order) of every BatchNorm case: (forward, backward)
BN_RECORDS = {
    "bn_bf16_bf16_M1_C8": ((1, 8, 1, 256, 256, 1, 1, 0), (1, 8, 1, 256, 256, 1, 1, 0)),
    "bn_bf16_bf16_M257_C8": ((1, 8, 1, 256, 256, 2, 1, 0), (1, 8, 1, 256, 256, 2, 1, 0)),
    "bn_f32_f32_M511_C12_offset": ((1, 4, 3, 85, 85, 7, 3, 0), (1, 4, 3, 85, 85, 7, 3, 0)),
    "bn_f32_f32_M2721_C12": ((1, 4, 3, 85, 85, 33, 9, 0), (1, 4, 3, 85, 85, 33, 9, 0)),
    "bn_f32_f32_M5_C80": ((1, 4, 20, 12, 12, 1, 5, 0), (1, 4, 20, 12, 12, 1, 5, 0)),
    "bn_f32_f32_M85_C80_noaffine": ((1, 4, 20, 12, 12, 8, 5, 0), (1, 4, 20, 12, 12, 8, 5, 0)),
    "bn_f32_f32_M85_C80_constant": ((1, 4, 20, 12, 12, 8, 5, 0), (1, 4, 20, 12, 12, 8, 5, 0)),
    "bn_f32_f32_M97_C80_offset": ((1, 4, 20, 12, 12, 9, 5, 0), (1, 4, 20, 12, 12, 9, 5, 0)),
    "bn_f32_bf16_M97_C80": ((1, 4, 20, 12, 12, 9, 5, 0), (1, 4, 20, 12, 12, 9, 5, 0)),
    "bn_f32_f32_M373_C80": ((1, 4, 20, 12, 12, 32, 10, 0), (1, 4, 20, 12, 12, 32, 10, 0)),
    "bn_f32_f32_M3049_C80_first_outlier": ((1, 4, 20, 12, 24, 128, 60, 0), (1, 4, 20, 12, 24, 128, 60, 0)),
    "bn_bf16_bf16_M151_C80": ((1, 8, 10, 25, 25, 7, 5, 0), (1, 8, 10, 25, 25, 7, 5, 0)),
    "bn_bf16_bf16_M776_C80_offset": ((1, 8, 10, 25, 25, 32, 10, 0), (1, 8, 10, 25, 25, 32, 10, 0)),
    "bn_bf16_bf16_M3_C512": ((1, 8, 64, 4, 4, 1, 1, 0), (1, 8, 64, 4, 4, 1, 1, 0)),
    "bn_bf16_bf16_M33_C512_norun": ((1, 8, 64, 4, 4, 9, 3, 0), (1, 8, 64, 4, 4, 9, 3, 0)),
    "bn_bf16_f32_M33_C512": ((1, 8, 64, 4, 4, 9, 3, 0), (0, 0, 0, 4, 512, 1, 66, 64)),
    "bn_bf16_bf16_M509_C512_constant": ((1, 8, 64, 4, 4, 128, 32, 0), (1, 8, 64, 4, 4, 128, 32, 0)),
    "bn_bf16_bf16_M1021_C512_first_outlier": ((1, 8, 64, 4, 8, 128, 64, 0), (1, 8, 64, 4, 8, 128, 64, 0)),
    "bn_bf16_bf16_M129_C2048": ((1, 8, 256, 1, 2, 65, 33, 0), (1, 8, 256, 1, 2, 65, 33, 0)),
    "bn_f32_f32_M129_C1024": ((1, 4, 256, 1, 2, 65, 33, 0), (1, 4, 256, 1, 2, 65, 33, 0)),
    "bn_f32_f32_M129_C1024_offset": ((1, 4, 256, 1, 2, 65, 33, 0), (1, 4, 256, 1, 2, 65, 33, 0)),
    "bn_f32_f32_M4_C1": ((2, 4, 1, 256, 256, 1, 1, 0), (2, 4, 1, 256, 256, 1, 1, 0)),
    "bn_bf16_bf16_M8_C1": ((2, 8, 1, 256, 256, 1, 1, 0), (2, 8, 1, 256, 256, 1, 1, 0)),
    "bn_f32_f32_M131076_C1_first_outlier": ((2, 4, 1, 256, 512, 65, 33, 0), (2, 4, 1, 256, 512, 65, 33, 0)),
    "bn_f32_bf16_M1028_C1": ((2, 4, 1, 256, 256, 2, 1, 0), (2, 4, 1, 256, 256, 2, 1, 0)),
    "bn_f32_f32_M1028_C1_offset": ((2, 4, 1, 256, 256, 2, 1, 0), (2, 4, 1, 256, 256, 2, 1, 0)),
    "bn_bf16_bf16_M2400_C1": ((2, 8, 1, 256, 256, 2, 1, 0), (2, 8, 1, 256, 256, 2, 1, 0)),
    "bn_f32_f32_M45_C1": ((0, 0, 0, 256, 8192, 1, 1, 1), (0, 0, 0, 256, 8192, 1, 1, 1)),
    "bn_f32_bf16_M45_C1": ((0, 0, 0, 256, 8192, 1, 1, 1), (0, 0, 0, 256, 8192, 1, 1, 1)),
    "bn_bf16_bf16_M45_C1": ((0, 0, 0, 256, 8192, 1, 1, 1), (0, 0, 0, 256, 8192, 1, 1, 1)),
    "bn_bf16_f32_M45_C1": ((0, 0, 0, 256, 8192, 1, 1, 1), (0, 0, 0, 256, 8192, 1, 1, 1)),
    "bn_f32_f32_M8193_C1": ((0, 0, 0, 256, 8192, 2, 33, 1), (0, 0, 0, 256, 8192, 2, 33, 1)),
    "bn_f32_f32_M37_C65": ((0, 0, 0, 4, 512, 1, 10, 64), (0, 0, 0, 4, 512, 1, 10, 64)),
    "bn_f32_bf16_M37_C65": ((0, 0, 0, 4, 512, 1, 10, 64), (0, 0, 0, 4, 512, 1, 10, 64)),
    "bn_f32_f32_M37_C65_noaffine_norun": ((0, 0, 0, 4, 512, 1, 10, 64), (0, 0, 0, 4, 512, 1, 10, 64)),
    "bn_f32_f32_M37_C65_offset": ((0, 0, 0, 4, 512, 1, 10, 64), (0, 0, 0, 4, 512, 1, 10, 64)),
    "bn_f32_f32_M37_C65_constant": ((0, 0, 0, 4, 512, 1, 10, 64), (0, 0, 0, 4, 512, 1, 10, 64)),
    "bn_f32_f32_M37_C65_first_outlier": ((0, 0, 0, 4, 512, 1, 10, 64), (0, 0, 0, 4, 512, 1, 10, 64)),
    "bn_f32_f32_M1_C65": ((0, 0, 0, 4, 512, 1, 1, 64), (0, 0, 0, 4, 512, 1, 1, 64)),
    "bn_bf16_bf16_M100_C12": ((0, 0, 0, 4, 512, 1, 5, 64), (0, 0, 0, 4, 512, 1, 5, 64)),
    "bn_bf16_bf16_M9_C2056": ((0, 0, 0, 4, 512, 1, 73, 64), (0, 0, 0, 4, 512, 1, 73, 64)),
    "bn_f32_f32_M9_C1028": ((0, 0, 0, 4, 512, 1, 37, 64), (0, 0, 0, 4, 512, 1, 37, 64)),
    "bn_f32_f32_M60_C1_misaligned": ((0, 0, 0, 256, 8192, 1, 1, 1), (0, 0, 0, 256, 8192, 1, 1, 1)),
    "bn_bf16_bf16_M64_C1_misaligned": ((0, 0, 0, 256, 8192, 1, 1, 1), (0, 0, 0, 256, 8192, 1, 1, 1)),
    "bn_f32_f32_M85_C80_misaligned": ((0, 0, 0, 4, 512, 1, 27, 64), (0, 0, 0, 4, 512, 1, 27, 64)),
    "bn_f32_bf16_M97_C80_misaligned": ((0, 0, 0, 4, 512, 1, 31, 64), (0, 0, 0, 4, 512, 1, 31, 64)),
    "bn_f32_f32_M37_C65_misaligned": ((0, 0, 0, 4, 512, 1, 10, 64), (0, 0, 0, 4, 512, 1, 10, 64)),
}

_F, _H = "f32", "bf16"

# (B, T, lens): forward rows = 1 (mod 4) -- the last block holds one row -- and a single row
_FWD_ROWS = [(3, 7, None), (5, 5, "mixed"), (1, 1, None), (7, 11, "zero_mid"), (3, 3, "one"), (5, 5, "full"),
             (3, 7, "zero_first")]
_PROFILES = ["plain", "offset", "constant", "tiny"]


def _ln_forward():
    out, i = [], 0

    def add(entry, tx, tr, ty, **kw):
        nonlocal i
        for D in (256, 512):
            B, T, lens = _FWD_ROWS[i % len(_FWD_ROWS)]
            out.append(ln_case(entry, B, T, D, tx, tr, ty, lens=lens, profile=_PROFILES[i % 4], **kw))
            i += 1
    for tx, ty in ((_H, _H), (_F, _F), (_H, _F), (_F, _H)):  # vo_layernorm: 4 I/O pairs, with and without res
        add("fwd", tx, tx, ty)
        add("fwd", tx, tx, ty, res=False)
    for tx, tr in ((_F, _F), (_H, _H), (_H, _F)):  # vo_layernorm_dual
        add("dual", tx, tr, _F)
    ps = [0.1, 0.5, 0.0]
    for j, (tx, tr, ty, y16) in enumerate(((_H, _F, _F, True), (_F, _F, _F, True), (_F, _F, _F, False),
                                           (_H, _H, _H, False), (_H, _F, _F, False))):  # vo_layernorm_drop
        for D in (256, 512):
            B, T, lens = _FWD_ROWS[i % len(_FWD_ROWS)]
            out.append(ln_case("drop", B, T, D, tx, tr, ty, y16=y16, p=ps[i % 3], lens=lens, profile=_PROFILES[i % 4]))
            i += 1
    return out


# backward: (B, T, lens) with rows = 64 (nblk - 1) + 1 -- the last workgroup holds one row, its other waves are
# dead -- for nblk = 1, 16, 17, 48, 49, 64, 65, 113 (ln_partial_sum_kernel's 4 x 16 unroll), and 21 rows
_N1, _N1B, _N16, _N16F = (1, 1, None), (3, 7, "mixed"), (31, 31, None), (31, 31, "full")
_N17, _N17Z, _N48, _N49 = (5, 205, "zero_mid"), (25, 41, "zero_first"), (17, 177, "mixed"), (7, 439, "one")
_N64, _N65, _N113 = (37, 109, "mixed"), (17, 241, "zero_first"), (67, 107, "mixed")


def _bw(entry, rows, D, tx, tr, tg, profile="plain", **kw):
    B, T, lens = rows
    return ln_case(entry, B, T, D, tx, tr, tg, lens=lens, profile=profile, **kw)


LN_CASES = _ln_forward() + [
    ln_case("fwd", 9, 57, 256, _H, _H, _H, lens="zero_mid"),  # 513 rows: one wrong row is 0.5 % of the tensor

    # vo_layernorm_bwd: (x, gy) dtypes, res of x's dtype
    _bw("bwd", _N17, 256, _H, _H, _H), _bw("bwd", _N1, 512, _H, _H, _H, "offset"),
    _bw("bwd", _N113, 256, _H, _H, _F, "tiny"), _bw("bwd", _N16, 512, _H, _H, _F, "constant"),
    _bw("bwd", _N16F, 256, _F, _F, _F, "offset"), _bw("bwd", _N48, 512, _F, _F, _F),
    _bw("bwd", _N49, 256, _F, _F, _H, "constant"), _bw("bwd", _N1B, 512, _F, _F, _H, "tiny"),
    _bw("bwd", _N17Z, 256, _F, _F, _F, res=False), _bw("bwd", _N16, 256, _H, _H, _H, res=False),
    # vo_layernorm_bwd_ex: bf16 x, fp32 res, gy fp32 / bf16, with and without gy2; gh32 beside gh
    _bw("bwd_ex", _N64, 256, _H, _F, _F), _bw("bwd_ex", _N17, 512, _H, _F, _F, "offset"),
    _bw("bwd_ex", _N17Z, 256, _H, _F, _F, gy2=True), _bw("bwd_ex", _N16, 512, _H, _F, _F, "tiny", gy2=True),
    _bw("bwd_ex", _N65, 256, _H, _F, _H, "constant"), _bw("bwd_ex", _N1B, 512, _H, _F, _H),
    _bw("bwd_ex", _N16F, 256, _H, _F, _H, "offset", gy2=True), _bw("bwd_ex", _N17, 512, _H, _F, _H, gy2=True),
    # ... without gh32; and res of x's dtype without gy2 and gh32: the forms it shares with vo_layernorm_bwd
    _bw("bwd_ex", _N17Z, 256, _H, _F, _F, gres=False), _bw("bwd_ex", _N1B, 512, _H, _F, _F, gy2=True, gres=False),
    _bw("bwd_ex", _N16, 256, _H, _F, _H, gres=False), _bw("bwd_ex", _N17, 512, _H, _F, _H, gy2=True, gres=False),
    _bw("bwd_ex", _N1B, 256, _H, _H, _H, gres=False), _bw("bwd_ex", _N17, 512, _H, _H, _F, gres=False),
    _bw("bwd_ex", _N16, 256, _F, _F, _F, gres=False), _bw("bwd_ex", _N17Z, 512, _F, _F, _H, gres=False),
    # vo_layernorm_bwd_drop
    _bw("bwd_drop", _N17Z, 256, _H, _F, _F, p=0.1, gy2=True), _bw("bwd_drop", _N16, 512, _H, _F, _F, "offset", p=0.5),
    _bw("bwd_drop", _N48, 256, _H, _F, _H, "tiny", p=0.5), _bw("bwd_drop", _N17, 512, _H, _F, _H, p=0.0, gy2=True),
    _bw("bwd_drop", _N1B, 256, _H, _F, _F, p=0.0), _bw("bwd_drop", _N1B, 512, _H, _F, _H, "constant", p=0.1),
    _bw("bwd_drop", _N16F, 256, _F, _F, _F, p=0.1), _bw("bwd_drop", _N49, 512, _F, _F, _F, "constant", p=0.5),
    _bw("bwd_drop", _N113, 256, _H, _H, _H, p=0.1), _bw("bwd_drop", _N1, 512, _H, _H, _H, "offset", p=0.5),
]

BN_CASES = [
    # vectorised route: CV = C / V vector columns, RL = 256 / CV row lanes; M chosen for nb and a one-row last block
    bn_case(1, 8, _H), bn_case(257, 8, _H),                                      # CV 1, RL 256
    bn_case(511, 12, _F, profile="offset"), bn_case(2721, 12, _F),               # CV 3, RL 85: nb 7, 33
    bn_case(5, 80, _F), bn_case(85, 80, _F, affine=False), bn_case(85, 80, _F, profile="constant"),
    bn_case(97, 80, _F, profile="offset"), bn_case(97, 80, _F, _H), bn_case(373, 80, _F),
    bn_case(3049, 80, _F, profile="first_outlier"),                              # CV 20, RL 12, 16 idle threads
    bn_case(151, 80, _H), bn_case(776, 80, _H, profile="offset"),                # CV 10, RL 25: nb 7, 32
    bn_case(3, 512, _H), bn_case(33, 512, _H, running=False), bn_case(33, 512, _H, _F),
    bn_case(509, 512, _H, profile="constant"), bn_case(1021, 512, _H, profile="first_outlier"),
    bn_case(129, 2048, _H), bn_case(129, 1024, _F), bn_case(129, 1024, _F, profile="offset"),  # CV 256, RL 1
    # FLAT route (C = 1): one vector, many blocks, fp32 x with bf16 dy
    bn_case(4, 1, _F), bn_case(8, 1, _H), bn_case(4 * (256 * 128 + 1), 1, _F, profile="first_outlier"),
    bn_case(1028, 1, _F, _H), bn_case(1028, 1, _F, profile="offset"), bn_case(2400, 1, _H),
    # scalar route
    bn_case(45, 1, _F), bn_case(45, 1, _F, _H), bn_case(45, 1, _H), bn_case(45, 1, _H, _F), bn_case(8193, 1, _F),
    bn_case(37, 65, _F), bn_case(37, 65, _F, _H), bn_case(37, 65, _F, affine=False, running=False),
    bn_case(37, 65, _F, profile="offset"), bn_case(37, 65, _F, profile="constant"),
    bn_case(37, 65, _F, profile="first_outlier"), bn_case(1, 65, _F),
    bn_case(100, 12, _H), bn_case(9, 2056, _H), bn_case(9, 1028, _F),
    # a contiguous view that starts 60 bytes into its allocation takes the scalar kernels, whatever its shape
    bn_case(60, 1, _F, misaligned=True), bn_case(64, 1, _H, misaligned=True), bn_case(85, 80, _F, misaligned=True),
    bn_case(97, 80, _F, _H, misaligned=True), bn_case(37, 65, _F, misaligned=True),
]

for _c in BN_CASES:
    _c["rec_fwd"], _c["rec_bwd"] = BN_RECORDS.get(_c["name"], (None, None))
CASES = LN_CASES + BN_CASES
for _c in CASES:
    _c["ill"] = STANDIN_REL_L2.get(_c["name"])


def _ln_required():
    req = set()
    for npl in (4, 8):
        for tx, ty in ((_H, _H), (_F, _F), (_H, _F), (_F, _H)):                   # vo_layernorm
            req.add(("layernorm_kernel", tx, tx, ty, npl, False, False, False, False))
            req.add(("layernorm_kernel/nores", tx, ty, npl))
        for tx, tr in ((_F, _F), (_H, _H), (_H, _F)):                             # vo_layernorm_dual
            req.add(("layernorm_kernel", tx, tr, _F, npl, True, False, False, False))
        for tx, tr, ty, dual in ((_H, _F, _F, True), (_F, _F, _F, True), (_F, _F, _F, False), (_H, _H, _H, False),
                                 (_H, _F, _F, False)):                            # vo_layernorm_drop
            req.add(("layernorm_kernel", tx, tr, ty, npl, dual, True, False, False))
        for tx, tg in ((_H, _H), (_H, _F), (_F, _F), (_F, _H)):                   # vo_layernorm_bwd
            req.add(("layernorm_bwd_kernel", tx, tx, tg, npl, False, False, False, False))
        for tg in (_F, _H):                                                       # vo_layernorm_bwd_ex
            for gy2 in (False, True):
                req.add(("layernorm_bwd_kernel", _H, _F, tg, npl, False, False, gy2, True))
        for tx, tr, tg in ((_H, _F, _F), (_H, _F, _H), (_F, _F, _F), (_H, _H, _H)):  # vo_layernorm_bwd_drop
            req.add(("layernorm_bwd_kernel", tx, tr, tg, npl, False, True, False, True))
    # ... and its two forms that take gy2
    req.add(("layernorm_bwd_kernel", _H, _F, _F, 4, False, True, True, True))
    req.add(("layernorm_bwd_kernel", _H, _F, _H, 8, False, True, True, True))
    return req


REQUIRED = _ln_required() | {
    # every bn_* instantiation reachable from vo_bn_train_fwd / vo_bn_bwd
    ("bn_stats_kernel", _F, 1), ("bn_stats_kernel", _F, 64), ("bn_stats_kernel", _H, 1), ("bn_stats_kernel", _H, 64),
    ("bn_finalize_kernel",), ("bn_apply_kernel", _F), ("bn_apply_kernel", _H),
    ("bn_bwd_stats_kernel", _F, _F, 1), ("bn_bwd_stats_kernel", _F, _F, 64), ("bn_bwd_stats_kernel", _F, _H, 1),
    ("bn_bwd_stats_kernel", _F, _H, 64), ("bn_bwd_stats_kernel", _H, _F, 1), ("bn_bwd_stats_kernel", _H, _F, 64),
    ("bn_bwd_stats_kernel", _H, _H, 1), ("bn_bwd_stats_kernel", _H, _H, 64), ("bn_bwd_finalize_kernel",),
    ("bn_bwd_apply_kernel", _F, _F), ("bn_bwd_apply_kernel", _F, _H), ("bn_bwd_apply_kernel", _H, _F),
    ("bn_bwd_apply_kernel", _H, _H),
    ("bn_stats_v_kernel", _F, False), ("bn_stats_v_kernel", _F, True), ("bn_stats_v_kernel", _H, False),
    ("bn_stats_v_kernel", _H, True), ("bn_finalize_v_kernel",),
    ("bn_apply_v_kernel", _F, False), ("bn_apply_v_kernel", _F, True), ("bn_apply_v_kernel", _H, False),
    ("bn_apply_v_kernel", _H, True),
    ("bn_bwd_stats_v_kernel", _F, _F, False), ("bn_bwd_stats_v_kernel", _F, _F, True),
    ("bn_bwd_stats_v_kernel", _F, _H, False), ("bn_bwd_stats_v_kernel", _F, _H, True),
    ("bn_bwd_stats_v_kernel", _H, _H, False), ("bn_bwd_stats_v_kernel", _H, _H, True),
    ("bn_bwd_finalize_v_kernel",), ("bn_bwd_finalize_flat_kernel",),
    ("bn_bwd_apply_v_kernel", _F, _F, False), ("bn_bwd_apply_v_kernel", _F, _F, True),
    ("bn_bwd_apply_v_kernel", _F, _H, False), ("bn_bwd_apply_v_kernel", _F, _H, True),
    ("bn_bwd_apply_v_kernel", _H, _H, False), ("bn_bwd_apply_v_kernel", _H, _H, True),
    # edges
    *(f"ln_bwd/nblk/{n}" for n in (1, 16, 17, 48, 49, 64, 65, 113)), "ln_bwd/last_block_one_row", "ln_bwd/row0_is_pad",
    "ln_fwd/rows%4==1", "ln_fwd/one_row",
    *(f"ln/lens/{s}" for s in (None, "full", "one", "zero_mid", "mixed", "zero_first")),
    *(f"ln/profile/{s}" for s in _PROFILES), *(f"ln/p/{p}" for p in (0.0, 0.1, 0.5)),
    *(f"bn_vec/nb/{n}" for n in (1, 7, 8, 9, 32, 33, 128)), *(f"bn_vec/CV/{n}" for n in (1, 3, 10, 20, 64, 256)),
    "bn_vec/idle_threads/16", "bn_vec/idle_threads/1", "bn_vec/idle_threads/6", "bn_vec/last_block_one_row",
    "bn_flat/one_vector/f32", "bn_flat/one_vector/bf16", "bn_flat/nb/65", "bn_flat/nb/2",
    "bn_scalar/one_channel_tile", "bn_scalar/past_vector_limit/f32", "bn_scalar/past_vector_limit/bf16",
    "bn_bwd/bf16_x_f32_dy_falls_back",
    *(f"bn_misaligned/{k}/{w}" for k in ("flat", "vec") for w in ("fwd", "bwd")),
    *(f"bn/profile/{s}" for s in ("plain", "offset", "constant", "first_outlier")), "bn/M1", "bn/no_affine",
    "bn/no_running",
}


# ---------------------------------------------------------------------------------------------- GPU runners

def _dt(t):
    from visual_onoma_to_wave_amd import ops
    return ops.vo_dtype(t)


def _call_ln(c, m, d, B=None, D=None):
    """The C entry point of a LayerNorm case on pointers into the guarded device buffers ``d``; returns its status.
    B / D: passed in place of the case's (a refused size: the buffers keep the case's)."""
    from visual_onoma_to_wave_amd import _lib
    L = _lib.lib()
    B, T, D = c["B"] if B is None else B, c["T"], c["D"] if D is None else D

    def v(name):
        return NC.view(m, name, d) if name in m["spec"] else None

    def p(name):
        t = v(name)
        return None if t is None else ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, res = v("x"), v("res")
    e = c["entry"]
    rdt = _dt(res) if res is not None else _dt(x)
    if e == "fwd":
        return L.vo_layernorm(p("x"), _dt(x), p("res"), rdt, p("gamma"), p("beta"), p("lens"), B, T, D, NC.EPS,
                              p("y"), _dt(v("y")), st)
    if e == "dual":
        return L.vo_layernorm_dual(p("x"), _dt(x), p("res"), rdt, p("gamma"), p("beta"), p("lens"), B, T, D, NC.EPS,
                                   p("y"), p("y16"), st)
    if e == "drop":
        return L.vo_layernorm_drop(p("x"), _dt(x), p("res"), rdt, p("gamma"), p("beta"), p("lens"), B, T, D, NC.EPS,
                                   p("y"), _dt(v("y")), p("y16"), c["p"], p("seed"), c["salt"], st)
    if e == "bwd":
        return L.vo_layernorm_bwd(p("x"), p("res"), _dt(x), p("gy"), _dt(v("gy")), p("gamma"), p("lens"), B, T, D,
                                  NC.EPS, p("gh"), p("dgamma"), p("dbeta"), p("ws"), st)
    if e == "bwd_ex":
        return L.vo_layernorm_bwd_ex(p("x"), _dt(x), p("res"), rdt, p("gy"), _dt(v("gy")), p("gy2"), p("gamma"),
                                     p("lens"), B, T, D, NC.EPS, p("gh"), p("gres"), p("dgamma"), p("dbeta"),
                                     p("ws"), st)
    return L.vo_layernorm_bwd_drop(p("x"), _dt(x), p("res"), rdt, p("gy"), _dt(v("gy")), p("gy2"), p("gamma"),
                                   p("lens"), B, T, D, NC.EPS, c["p"], p("seed"), c["salt"], p("gh"), p("gres"),
                                   p("dgamma"), p("dbeta"), p("ws"), st)


def _run_ln(c, m, d):
    """The C entry point on pointers into the guarded device buffers ``d``; then the ops wrapper, bit for bit."""
    from visual_onoma_to_wave_amd import _lib, ops
    B, T, D = c["B"], c["T"], c["D"]

    def v(name):
        return NC.view(m, name, d) if name in m["spec"] else None
    _lib.check(_call_ln(c, m, d), c["name"])
    x, res, lens, gamma = v("x"), v("res"), v("lens"), v("gamma")
    x3 = x.view(B, T, D)
    r3 = None if res is None else res.view(B, T, D)
    g2 = None if v("gy2") is None else v("gy2").view(B, T, D)
    e = c["entry"]
    if e == "fwd":
        w = dict(y=ops.layernorm(x3, gamma, v("beta"), res=r3, lens=lens, out_dtype=v("y").dtype, eps=NC.EPS))
    elif e == "dual":
        w = dict(zip(("y", "y16"), ops.layernorm(x3, gamma, v("beta"), res=r3, lens=lens, out_dtype=torch.float32,
                                                 eps=NC.EPS, with_bf16=True)))
    elif e == "drop":
        o = ops.layernorm_drop(x3, gamma, v("beta"), r3, c["p"], v("seed"), c["salt"], lens=lens,
                               with_bf16=c["dual"], eps=NC.EPS)
        w = dict(zip(("y", "y16"), o)) if c["dual"] else dict(y=o)
    elif e == "bwd":
        w = dict(zip(("gh", "dgamma", "dbeta"),
                     ops.layernorm_bwd(x3, v("gy").view(B, T, D), gamma, res=r3, lens=lens, eps=NC.EPS)))
    elif e == "bwd_ex" and c["tx"] == c["tr"]:  # ops.layernorm_bwd_ex takes bf16 x with fp32 res only: the same launch
        w = dict(zip(("gh", "dgamma", "dbeta"),
                     ops.layernorm_bwd(x3, v("gy").view(B, T, D), gamma, res=r3, lens=lens, eps=NC.EPS)))
    elif e == "bwd_ex":
        w = dict(zip(("gh", "gres", "dgamma", "dbeta"),
                     ops.layernorm_bwd_ex(x3, v("gy").view(B, T, D), gamma, r3, lens=lens, gy2=g2, eps=NC.EPS)))
        if not c["gres"]:  # the wrapper always passes a gh32
            del w["gres"]
    else:
        w = dict(zip(("gh", "gres", "dgamma", "dbeta"),
                     ops.layernorm_bwd_drop(x3, v("gy").view(B, T, D), gamma, r3, c["p"], v("seed"), c["salt"],
                                            lens=lens, gy2=g2, eps=NC.EPS)))
    return w


def _run_bn(c, m, d):
    from visual_onoma_to_wave_amd import _lib, ops
    L = _lib.lib()
    M, C = c["M"], c["C"]

    def v(name):
        return NC.view(m, name, d) if name in m["spec"] else None

    def p(name):
        t = v(name)
        return None if t is None else ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, dy = v("x"), v("dy")
    # the route of the very pointers about to be passed: the declared record, and for a misaligned view scalar
    ptrs = {k: v(k).data_ptr() for k in ("x", "dy", "y", "dx")}
    assert (ptrs["x"] % 16 != 0) == c["misaligned"] and (ptrs["y"] % 16 != 0) == c["misaligned"]
    for which in ("fwd", "bwd"):
        got = ops.bn_route(*NC.route_args(c, which, ptrs))
        assert got == NC.record(c, which), (c["name"], which, got)
        assert not c["misaligned"] or got["route"] == NC.SCALAR, (c["name"], which, got)
    run0 = {k: v(k).clone() for k in ("run_mean", "run_var", "nbt") if k in m["spec"]}
    _lib.check(L.vo_bn_train_fwd(p("x"), _dt(x), M, C, p("gamma"), p("beta"), c["eps"], c["momentum"], p("run_mean"),
                                 p("run_var"), p("nbt"), p("mean_rstd"), p("ws_fwd"), p("y"), st), c["name"])
    _lib.check(L.vo_bn_bwd(p("x"), _dt(x), p("dy"), _dt(dy), M, C, p("gamma"), p("mr_in"), p("ws_bwd"), p("dgamma"),
                           p("dbeta"), p("dx"), st), c["name"])
    y, mr = ops.bn_train_fwd(x, v("gamma"), v("beta"), c["eps"], c["momentum"], run0.get("run_mean"),
                             run0.get("run_var"), run0.get("nbt"))
    dx, dg, db = ops.bn_bwd(x, dy, v("gamma"), v("mr_in"))
    w = dict(y=y, mean_rstd=mr, dx=dx, dgamma=dg, dbeta=db)
    w.update(run0)
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_norm_case(c):
    from visual_onoma_to_wave_amd import _lib, ops
    dev = torch.device("cuda")
    mask = None
    if c["kind"] == "ln" and c["drop"]:  # vo_dropout's draw for the same (seed, salt)
        seed = torch.tensor([NC.seed_value(c)], dtype=torch.int64, device=dev)
        mask = ops.dropout(torch.ones(c["B"] * c["T"], c["D"], device=dev), c["p"], seed, c["salt"]) != 0
        n = mask.numel()  # the kept share, to four standard deviations of a fair draw
        assert abs(float(mask.float().mean()) - (1 - c["p"])) <= 4 * (c["p"] * (1 - c["p"]) / n) ** 0.5
    m = NC.make(c, mask)
    if c["kind"] == "bn":
        NC.add_workspace(c, m, int(_lib.lib().vo_bn_workspace_size(c["M"], c["C"])))
    ref = NC.reference(c, m)
    d = {k: b.to(dev) for k, b in m["bufs"].items()}
    w = (_run_ln if c["kind"] == "ln" else _run_bn)(c, m, d)
    torch.cuda.synchronize()
    for k, t in w.items():  # the wrapper's result: bit for bit the direct call's
        assert torch.equal(NC._bits(t.reshape(-1)), NC._bits(NC.view(m, k, d).reshape(-1))), f"{c['name']}: wrapper {k}"
    m["bufs"] = {k: b.cpu() for k, b in d.items()}
    NC.verify(c, m, ref)


# ---------------------------------------------------------------------------------------------- refusals

_ENTRY_NAME = {"fwd": b"layernorm", "dual": b"layernorm_dual", "drop": b"layernorm_drop", "bwd": b"layernorm_bwd",
               "bwd_ex": b"layernorm_bwd_ex", "bwd_drop": b"layernorm_bwd_drop"}
VO_ERR_INVALID = -1  # include/vonoma.h


def _refusal_case(entry, combo):
    """B = 2, T = 3, D = 256, lens [3, 1]: one call of NC.ln_domain as a case (guards around every output)."""
    tx, tr, t3, aux, gres = combo
    bwd = entry.startswith("bwd")
    return ln_case(entry, 2, 3, 256, tx, tr, t3, lens=(3, 1), p=0.1 if entry in ("drop", "bwd_drop") else None,
                   gy2=bwd and aux, y16=(not bwd) and aux, gres=gres if bwd else None)


def _assert_refused(c, m, d, **size):
    """VO_ERR_INVALID, the error names the entry, and no buffer changed: outputs and guards keep their patterns."""
    from visual_onoma_to_wave_amd import _lib
    rc = _call_ln(c, m, d, **size)
    err = _lib.lib().vo_last_error()
    assert rc == VO_ERR_INVALID, (c["name"], size, rc)
    assert err.startswith(_ENTRY_NAME[c["entry"]] + b":"), (c["name"], size, err)
    torch.cuda.synchronize()
    for k, b in d.items():
        assert torch.equal(NC._bits(b.cpu()), NC._bits(m["bufs"][k])), (c["name"], size, k)


@pytest.mark.gpu
def test_layernorm_entries_refuse_every_call_outside_the_accept_table():
    """Every entry over every dtype of each of its dtype arguments, with and without y16 / gy2 / gh32: what
    NC.LN_ACCEPTS leaves out returns VO_ERR_INVALID before any launch; so do D = 128 and B = 0 on a call the entry
    takes.  (The accepted calls are the cases above: tests/test_norm_check.py.)"""
    dev = torch.device("cuda")
    refused = 0
    for entry in NC.LN_ENTRIES:
        sized = False
        for combo in NC.ln_domain(entry):
            c = _refusal_case(entry, combo)
            m = NC.make(c)
            d = {k: b.to(dev) for k, b in m["bufs"].items()}
            if combo not in NC.LN_ACCEPTS[entry]:
                _assert_refused(c, m, d)
                refused += 1
            elif not sized:
                _assert_refused(c, m, d, D=128)
                _assert_refused(c, m, d, B=0)
                sized = True
        assert sized, entry
    assert refused == 46


@pytest.mark.gpu
@pytest.mark.parametrize("wrapper", ["layernorm_bwd_ex", "layernorm_bwd_drop"])
def test_backward_wrappers_check_gy_res_and_gy2_before_any_launch(wrapper, monkeypatch):
    """An fp32 gy2 (the kernels read it as bf16: there is no dtype argument), and a gy2, gy or res of another shape:
    ValueError before the library is even looked up."""
    from visual_onoma_to_wave_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(5)
    x, gy2 = (torch.randn(2, 3, 256, device=dev, generator=g).bfloat16() for _ in range(2))
    res, gy = (torch.randn(2, 3, 256, device=dev, generator=g) for _ in range(2))
    gamma = torch.ones(256, device=dev)
    seed = torch.tensor([5], dtype=torch.int64, device=dev)

    def call(**kw):
        a = dict(x=x, gy=gy, res=res, gy2=gy2)
        a.update(kw)
        if wrapper == "layernorm_bwd_ex":
            return ops.layernorm_bwd_ex(a["x"], a["gy"], gamma, a["res"], gy2=a["gy2"])
        return ops.layernorm_bwd_drop(a["x"], a["gy"], gamma, a["res"], 0.1, seed, 3, gy2=a["gy2"])

    def other(t):
        return t[:, :2].contiguous()
    assert all(t.shape == x.shape for t in call()[:2])  # the call the bad ones are one step from

    def launched():
        raise AssertionError("reached the library")
    monkeypatch.setattr(ops._lib, "lib", launched)
    for bad in (dict(gy2=gy2.float()), dict(gy2=other(gy2)), dict(gy=other(gy)), dict(res=other(res))):
        with pytest.raises(ValueError, match=wrapper):
            call(**bad)
