"""Sample-rate conversion without a GPU: the library's host-only entries
(vo_resample_geometry, vo_resample_len, vo_resample_table) against the float64 yardstick tests/resample_check.py, the
yardstick against analytically sampled sines, the checker against its own mutations, and ``audio.read_wav``."""

import ctypes
import wave

import numpy as np
import pytest

import resample_check as R

TILE = 256  # RS_TILE of csrc/resample.hip (ops.RESAMPLE_TILE; tests/test_gpu_resample.py asserts the two agree)


@pytest.fixture(scope="module")
def L():
    from visual_onoma_to_wave_amd import _lib
    return _lib.lib()


def _geometry(L, a, b):
    O, M, W = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = L.vo_resample_geometry(a, b, ctypes.byref(O), ctypes.byref(M), ctypes.byref(W))
    return rc, (O.value, M.value, W.value)


def test_geometry(L):
    for pair in ((48000, 22050), (22050, 48000), (44100, 22050), (16000, 22050), (96000, 22050), (2, 1), (1, 2),
                 (3, 2), (7, 5)):
        rc, got = _geometry(L, *pair)
        assert rc == 0 and got == R.geometry(*pair)[:3], (pair, got)
    assert R.geometry(48000, 22050) == (320, 147, 148, 297) and R.geometry(22050, 48000) == (147, 320, 68, 137)
    for pair, msg in (((22050, 22050), "equal"), ((44101, 22050), "44101 / 22050"), ((48000, 5000), "48 / 5"),
                      ((0, 22050), ">= 1"), ((22050, -1), ">= 1")):
        rc, got = _geometry(L, *pair)
        text = L.vo_last_error().decode()
        assert rc == -1 and got == (-1, -1, -1), (pair, rc, got)
        assert msg in text, (pair, text)
    rc, _ = _geometry(L, 44101, 22050)
    text = L.vo_last_error().decode()
    assert "1024" in text and "<= 8" in text, text  # the limits, beside the reduced pair


def test_geometry_through_ops():
    from visual_onoma_to_wave_amd import audio, ops
    assert ops.resample_geometry(48000, 22050) == (320, 147, 148)
    with pytest.raises(ValueError, match="44101 / 22050"):
        ops.resample_geometry(44101, 22050)
    with pytest.raises(ValueError, match="equal"):
        ops.resample_geometry(22050, 22050)
    assert audio.resample_length(48000, 48000, 22050) == 22050 and audio.resample_length(7, 22050, 22050) == 7
    assert audio.resample_length(4801, 48000, 22050) == R.length(4801, 320, 147)
    assert audio.Resample(22050, 22050).geometry is None
    with pytest.raises(ValueError, match="48 / 5"):
        audio.Resample(48000, 5000)


def test_len(L):
    for O, M in ((320, 147), (147, 320), (2, 1), (1, 2), (7, 5)):
        for k in (0, 1, 2, 5):
            for d in (-1, 0, 1):
                n = k * O + d
                want = int(np.ceil(n * M / O)) if n > 0 else 0  # exact in double at these sizes
                assert L.vo_resample_len(n, O, M) == want == max(R.length(n, O, M), 0), (O, M, n)
        n = 2 ** 31 - 1
        assert L.vo_resample_len(n, O, M) == (n * M + O - 1) // O


@pytest.mark.parametrize("O, M", [(2, 1), (3, 2), (2, 3), (7, 5), (320, 147), (147, 320)])
def test_table(L, O, M):
    """|t32 - t64| <= 2^-24 |t64| (1 + 1e-6) + 1e-12: half an fp32 ulp, plus room for two double implementations of
    sin(pi t) and I0 disagreeing in their last bits.  Every row sums to 1 within 1e-6."""
    t64 = R.table64(O, M)
    t32 = np.full(t64.shape, np.nan, np.float32)
    assert L.vo_resample_table(O, M, t32.ctypes.data_as(ctypes.c_void_p)) == 0
    err = np.abs(t32.astype(np.float64) - t64)
    tol = 2.0 ** -24 * np.abs(t64) * (1 + 1e-6) + 1e-12
    worst = np.unravel_index(np.argmax(err - tol), err.shape)
    assert (err <= tol).all(), (worst, t32[worst], t64[worst])
    assert (t32[t64 == 0] == 0).all()
    sums = t32.astype(np.float64).sum(axis=1)
    print(f"({O}, {M}): row sums in 1 - {1 - sums.min():.2e} .. 1 - {1 - sums.max():.2e}")
    assert np.abs(sums - 1).max() <= 1e-6


def test_table_refusals(L):
    buf = np.full(4096, np.nan, np.float32)
    for O, M in ((4, 2), (1, 1), (9, 1), (1025, 1024), (0, 1), (2, -1)):
        assert L.vo_resample_table(O, M, buf.ctypes.data_as(ctypes.c_void_p)) == -1, (O, M)
        assert np.isnan(buf).all()
    assert L.vo_resample_table(2, 1, None) == -1


@pytest.mark.parametrize("sr_in, sr_out, hz", [(48000, 22050, 1000.0), (48000, 22050, 9000.0),
                                               (22050, 48000, 9000.0), (2, 1, 0.4), (3, 2, 0.8), (2, 3, 0.8),
                                               (7, 5, 2.0)])
def test_yardstick_passes_a_sine(sr_in, sr_out, hz):
    """A sine at or below 0.82 of the lower Nyquist, through ``model`` with a full-length row, is the analytically
    sampled sine within 1e-6 at outputs more than W M / O + 2 from either end (no package code involved)."""
    assert hz <= 0.82 * min(sr_in, sr_out) / 2
    O, M, W, T = R.geometry(sr_in, sr_out)
    n_in = 6 * W + 4 * O + 50
    x = np.sin(2 * np.pi * hz * np.arange(n_in) / sr_in + 0.3)
    N_out = R.length(n_in, O, M)
    # float64 samples: the yardstick's own error, without the fp32 rounding of the input
    r, xw = R._windows(x, n_in, np.arange(N_out), O, M, W, T)
    y64 = (R.table64(O, M)[r] * xw).sum(axis=1)
    want = np.sin(2 * np.pi * hz * np.arange(N_out) / sr_out + 0.3)
    edge = int(np.ceil(W * M / O)) + 2
    assert N_out > 2 * edge + 10
    err = np.abs(y64 - want)[edge:N_out - edge].max()
    print(f"{sr_in} -> {sr_out}, {hz} Hz: worst interior error {err:.2e}")
    assert err <= 1e-6


def test_yardstick_stops_a_sine_above_the_output_nyquist():
    """12 kHz at 48000 -> 22050 is 1.09 of the output Nyquist: at most 1e-6 of it is left in the interior."""
    O, M, W, T = R.geometry(48000, 22050)
    n_in = 6 * W + 4 * O + 50
    x = np.sin(2 * np.pi * 12000.0 * np.arange(n_in) / 48000 + 0.3)
    N_out = R.length(n_in, O, M)
    r, xw = R._windows(x, n_in, np.arange(N_out), O, M, W, T)
    y64 = (R.table64(O, M)[r] * xw).sum(axis=1)
    edge = int(np.ceil(W * M / O)) + 2
    left = np.abs(y64)[edge:N_out - edge].max()
    print(f"12 kHz at 48000 -> 22050: {left:.2e} left")
    assert left <= 1e-6


def _self_test_rows():
    """(x, n_b, skip, O, M, N_out) rows: per ratio the ragged noise rows of the GPU matrix (fp32 and int16), one of
    them with a skip, and the impulse rows."""
    rows = []
    for O, M in R.RATIOS:
        lens = R.row_lengths(O, M, TILE)
        N_out = R.length(max(lens), O, M) + 3
        for kind in ("float32", "int16"):
            x, _ = R.noise_batch(lens, kind, 100 * O + M)
            for b, n in enumerate(lens):
                rows.append((R.as_read(x[b]), n, 0, O, M, N_out))
        x, _ = R.noise_batch(lens, "float32", 100 * O + M)
        rows.append((x[-1], lens[-1], 3, O, M, N_out))
        xi, n_b, _ = R.impulse_rows(O, M)
        rows += [(xi[b], n_b, 0, O, M, R.length(n_b, O, M) + 3) for b in range(3)]
    return rows


def test_checker_passes_fp32_and_fails_every_mutation():
    rows = _self_test_rows()
    tables = {(O, M): R.table64(O, M) for O, M in R.RATIOS}
    caught = dict.fromkeys(R.MUTATIONS, 0)
    for x, n_b, skip, O, M, N_out in rows:
        h64 = tables[(O, M)]
        T = h64.shape[1]
        y64, S, m_b = R.model(x, n_b, skip, O, M, N_out, h64)
        y, m = R.emulate(x, n_b, skip, O, M, N_out, None, h64.astype(np.float32))
        assert m == m_b
        R.check(y, y64, S, m_b, T)
        for mut in R.MUTATIONS:
            y, m = R.emulate(x, n_b, skip, O, M, N_out, mut, h64.astype(np.float32))
            try:
                R.check(y, y64, S, m_b, T)
                assert m == m_b, "out_lens"
            except AssertionError:
                caught[mut] += 1
    assert all(caught.values()), caught
    # the dropped last tap is below the tolerance on noise: only impulse rows show it, as a whole output
    O, M = 3, 2
    h64 = tables[(O, M)]
    x, lens = R.noise_batch([700], "float32", 5)
    y64, S, m_b = R.model(x[0], 700, 0, O, M, 500, h64)
    y, _ = R.emulate(x[0], 700, 0, O, M, 500, "last_tap_dropped", h64.astype(np.float32))
    R.check(y, y64, S, m_b, h64.shape[1])


def test_guard_helpers():
    for dt in (np.float32, np.int16):
        buf = R.guarded(2, 5, dt)
        assert R.untouched(buf)
        R.check_guard(buf, 2, 5)
        buf[3] = 0
        assert not R.untouched(buf)
        R.check_guard(buf, 2, 5)
        buf[-1] = 0
        with pytest.raises(AssertionError, match="guard element 63"):
            R.check_guard(buf, 2, 5)


def _write_wav(path, data, rate, width=2):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1 if data.ndim == 1 else data.shape[1])
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(data.tobytes())


def test_read_wav(tmp_path):
    from visual_onoma_to_wave_amd.audio import read_wav
    rng = np.random.default_rng(0)
    mono = rng.integers(-32768, 32768, 1001).astype("<i2")
    _write_wav(tmp_path / "mono.wav", mono, 48000)
    got, rate = read_wav(tmp_path / "mono.wav")
    assert rate == 48000 and got.dtype == np.int16 and np.array_equal(got, mono)
    stereo = rng.integers(-32768, 32768, (77, 2)).astype("<i2")
    _write_wav(tmp_path / "stereo.wav", stereo, 44100)
    got, rate = read_wav(str(tmp_path / "stereo.wav"))
    want = (stereo.astype(np.float32) / np.float32(32768)).mean(axis=1, dtype=np.float32)
    assert rate == 44100 and got.dtype == np.float32 and got.shape == (77,) and np.array_equal(got, want)
    _write_wav(tmp_path / "eight.wav", rng.integers(0, 256, 50).astype(np.uint8), 8000, width=1)
    with pytest.raises(ValueError, match=r"eight\.wav.*8-bit"):
        read_wav(tmp_path / "eight.wav")
