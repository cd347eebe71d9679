"""Training batches of the vocoder on the device: aligned (mel, audio) segments cut from a
``dataset.DeviceCorpus`` with its waveforms attached, and the random draw of their rows from a counter in device
memory, so that a captured training step replays with its batch.

What this replaces is HiFi-GAN's ``MelDataset`` on the host (``random.randint`` per item, numpy crops,
``torch.from_numpy`` and a host-to-device copy per step).  ``mel="corpus"`` is its fine-tuning branch (the mel as the
acoustic model is trained to predict it, the audio cropped at ``mel_start * hop``), ``mel="audio"`` its from-scratch
branch (the training mel computed from the cropped audio).  include/vonoma.h states the rules of both kernels;
``segment_plan_host`` is the draw's rule in numpy.
"""

import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC 2011): four 32-bit counter words and two key words -> four output words."""
    c0, c1, c2, c3 = (int(v) & _U32 for v in counter)
    k0, k1 = (int(v) & _U32 for v in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _U32, (p0 >> 32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _W0) & _U32, (k1 + _W1) & _U32
    return c0, c1, c2, c3


def segment_plan_host(order, counter, seed, B, fps, n_frames):
    """``ops.segment_plan`` in numpy -> plan (B, 2) int32, rows ``src, start``: row b is drawn from k = counter + b,
    src = order[k mod len(order)]; (src, 0) for a src outside the corpus; otherwise start = (w * span) >> 32 with
    span = F - fps + 1 for F = n_frames[src] > fps, else 1, and w word 0 of Philox4x32-10 of the counter words
    (k lo, k hi, 0, 0) under the key (seed lo, seed hi).  The caller's counter then advances by B."""
    order = [int(v) for v in np.asarray(order).reshape(-1)]
    counter, seed, B, fps = int(counter), int(seed), int(B), int(fps)
    if not order or counter < 0 or not 0 <= seed < 2 ** 64 or B < 1 or fps < 1:
        raise ValueError(f"segment_plan_host: needs a non-empty order, counter >= 0, a seed in [0, 2^64), B >= 1 and "
                         f"fps >= 1, got ({len(order)} ids, {counter}, {seed}, {B}, {fps})")
    plan = np.zeros((B, 2), np.int32)
    for b in range(B):
        k = counter + b
        src = order[k % len(order)]
        start = 0
        if 0 <= src < len(n_frames):
            F = int(n_frames[src])
            span = F - fps + 1 if F > fps else 1
            w = philox4x32_10((k & _U32, (k >> 32) & _U32, 0, 0), (seed & _U32, seed >> 32))[0]
            start = (w * span) >> 32
        plan[b] = src, start
    return plan


def check_segment_plan(plan, n_frames, fps):
    """A host plan of ``ops.segment_batch`` -> int32 (B, 2), or ValueError naming the first row the kernel would
    refuse and the rule: src in [0, U), 0 <= start <= max(F - fps, 0)."""
    p = np.asarray(plan)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1 or p.dtype.kind not in "iu":
        raise ValueError(f"segment plan: must be integers of shape (B, 2) with B >= 1, rows src, start; got {p.dtype} "
                         f"{p.shape}")
    fps, U = int(fps), len(n_frames)
    if fps < 1:
        raise ValueError(f"segment plan: fps must be >= 1, got {fps}")
    for b, (src, start) in enumerate(p.tolist()):
        if not 0 <= src < U:
            raise ValueError(f"segment plan row {b}: src {src} is outside [0, {U})")
        last = max(int(n_frames[src]) - fps, 0)
        if not 0 <= start <= last:
            raise ValueError(f"segment plan row {b}: start {start} is outside [0, max(F - fps, 0)] = [0, {last}] "
                             f"(utterance {src} has F = {int(n_frames[src])} frames, fps = {fps})")
    return np.ascontiguousarray(p, np.int32)


class SegmentSampler:
    """Batches ``(x_mel_cl, y)`` for ``HifiGanTrainer.step`` drawn on the device from ``corpus`` (a ``DeviceCorpus``
    after ``attach_waves``): ``batch`` rows of ``segment_size`` samples and ``segment_size // hop`` frames per draw,
    utterances in the order of ``order`` (an int32 device tensor, 0 .. U - 1 at first; ``set_order`` writes an epoch's
    shuffle into it in place), the segment's start uniform among the positions that keep it inside the utterance (an
    utterance shorter than the segment starts at 0 and is padded: y with 0, x with ``mel_pad``).  The number of rows
    drawn so far is a counter in device memory (``position`` / ``seek``) that every draw advances, so a captured
    ``draw`` replays the following rows without the host (``HifiGanTrainer.step_graphed(sampler=...)``).

    ``mel="corpus"``: x is the corpus's mel of the segment.  ``mel="audio"``: x is the HiFi-GAN training mel of the
    drawn y, computed with ``h``'s n_fft, win_size, sampling_rate, fmin and fmax in one launch; ``mel_pad`` is unused.
    After a draw ``plan`` (batch, 2), ``frames`` and ``status`` (``_lib.SEG_*``) hold what was drawn."""

    def __init__(self, corpus, segment_size, hop, batch, seed=0, mel="corpus", h=None, mel_pad=0.0):
        import torch
        segment_size, hop, batch, seed = int(segment_size), int(hop), int(batch), int(seed)
        if getattr(corpus, "waves", None) is None:
            raise ValueError("SegmentSampler: the corpus has no waveforms (DeviceCorpus.attach_waves)")
        if hop < 1 or segment_size < hop or segment_size % hop != 0:
            raise ValueError(f"SegmentSampler: segment_size {segment_size} is not a multiple of hop {hop}")
        if hop != corpus.wave_hop:
            raise ValueError(f"SegmentSampler: hop {hop}, the waveforms were attached with hop {corpus.wave_hop}")
        if not 1 <= batch <= 65535:
            raise ValueError(f"SegmentSampler: batch must be in [1, 65535], got {batch}")
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"SegmentSampler: seed must be in [0, 2^64), got {seed}")
        if mel not in ("corpus", "audio"):
            raise ValueError(f"SegmentSampler: mel must be 'corpus' or 'audio', got {mel!r}")
        self.corpus, self.segment_size, self.hop, self.batch, self.seed = corpus, segment_size, hop, batch, seed
        self.fps, self.mel, self.mel_pad = segment_size // hop, mel, float(mel_pad)
        dev = corpus.device
        self.order = torch.arange(len(corpus), dtype=torch.int32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.plan = torch.zeros((batch, 2), dtype=torch.int32, device=dev)
        self.frames = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.status = torch.zeros(batch, dtype=torch.int32, device=dev)
        self._x = torch.zeros((batch, self.fps, corpus.n_mels), dtype=torch.float32, device=dev)
        self._y = torch.zeros((batch, segment_size), dtype=torch.float32, device=dev)
        self.n_mels = corpus.n_mels
        if mel == "audio":
            from ..audio import librosa_mel
            if h is None:
                raise ValueError("SegmentSampler: mel='audio' needs the vocoder's config h")
            if h.win_size != h.n_fft or h.hop_size != hop:
                raise ValueError(f"SegmentSampler: h has win_size {h.win_size}, n_fft {h.n_fft}, hop_size {h.hop_size} "
                                 f"(win_size == n_fft and hop_size == {hop})")
            self.n_fft, self.n_mels = int(h.n_fft), int(h.num_mels)
            fb = librosa_mel(h.sampling_rate, h.n_fft, h.num_mels, h.fmin, h.fmax)  # (n_mels, n_fft / 2 + 1)
            self.fb = torch.from_numpy(fb).t().contiguous().to(dev)
            self.window = torch.hann_window(h.win_size).to(dev)
            self._x_audio = torch.zeros((batch, self.fps, self.n_mels), dtype=torch.float32, device=dev)

    @property
    def epoch_steps(self):
        return -(-self.order.shape[0] // self.batch)

    def set_order(self, perm):
        """An epoch's utterance order (ids in [0, U), as many as the corpus has utterances), copied into ``order`` in
        place: the next draw, or replay, reads it."""
        import torch
        p = np.asarray(perm.cpu() if torch.is_tensor(perm) else perm).reshape(-1)
        if p.dtype.kind not in "iu" or p.size != self.order.shape[0] or int(p.min()) < 0 or int(p.max()) >= len(self.corpus):
            raise ValueError(f"SegmentSampler.set_order: {self.order.shape[0]} utterance ids in [0, {len(self.corpus)}) "
                             f"are needed, got {p.dtype} {p.shape}")
        self.order.copy_(torch.from_numpy(np.ascontiguousarray(p, np.int32)))
        return self

    def seek(self, k):
        """The next draw starts at row ``k`` of the sequence (in place: a replay follows)."""
        k = int(k)
        if not 0 <= k < 2 ** 63:
            raise ValueError(f"SegmentSampler.seek: k must be in [0, 2^63), got {k}")
        self.counter.fill_(k)
        return self

    def position(self):
        """Rows drawn so far (one device-to-host read)."""
        return int(self.counter.item())

    def draw(self, out=None):
        """The next ``batch`` rows -> (x_mel_cl (batch, fps, n_mels), y (batch, segment_size)), fp32 on the corpus's
        device: the plan kernel, then the batch kernel (then the mel kernel with ``mel="audio"``), on the current
        stream, nothing read on the host.  Without ``out`` the sampler's own static tensors are returned, overwritten
        by the next draw; ``out=(x, y)``: written in place."""
        from .. import ops
        x, y = (self._x_audio if self.mel == "audio" else self._x, self._y) if out is None else out
        ops.segment_plan(self.corpus.struct, self.order, self.counter, self.seed, self.batch, self.fps, plan=self.plan)
        xc = self._x if self.mel == "audio" else x
        ops.segment_batch(self.corpus.struct, self.corpus.waves, self.plan, self.fps, self.hop, self.mel_pad,
                          out={"y": y, "x": xc, "frames": self.frames, "status": self.status})
        if self.mel == "audio":
            ops.stft_mel_lens(y, self.window, self.fb, None, n_fft=self.n_fft, hop=self.hop,
                              pad=(self.n_fft - self.hop) // 2, mag_eps=1e-9, channels_last=True, want_energy=False,
                              mel=x)
        return x, y
