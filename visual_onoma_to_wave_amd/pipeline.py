"""Two-stage synthesis pipeline for serving on one GPU: glyph strips -> mel (vTTS) -> waveform
(HiFi-GAN), with the acoustic model of batch i + 1 on its own stream while the vocoder of batch i
runs on the caller's stream.

The acoustic model (``scripts/model/vtts.py:47-119``) is a chain of small, latency-bound kernels
at T_src = 12 / T_mel = 512 (2 ms for B = 32 alone, far from filling 256 CUs); the vocoder
(``scripts/hifigan/models.py:149-165``) fills the chip.  Overlapping them hides part of the
former behind the latter (bench.py: 13.67 -> 13.06 ms per B = 32 step).

Stream ordering.  ``submit`` first makes the acoustic stream wait for the caller's stream, so
inputs the caller produced there just before (``utils.tools.to_device`` lays glyph batches out
with a kernel on the current stream) are complete before the model reads them, and records every
CUDA input on the acoustic stream, so the caching allocator does not hand an input's memory out
while the acoustic model still reads it, even if the caller drops it right after ``submit``.
Each submitted batch's mel reaches the vocoder through an event; its memory is recorded on the
vocoder stream likewise.

``GraphedSynthesis`` is the low-latency counterpart: one request batch of a fixed shape bucket as one captured
graph from glyph strips to (int16) samples, replayed per call.
"""

import collections

import torch


class SynthesisPipeline:
    """``submit(*model_args, **model_kwargs)`` starts the acoustic model of a batch; ``next_wav()`` vocodes the
    oldest submitted batch on the current stream and returns (acoustic outputs, wav (B, N)).
    ``ragged``: the vocoder runs each batch with the acoustic model's own ``mel_len`` (``out[9]``, on the device:
    no host read) as ``Generator.run``'s ``lengths`` -- the padded frames are not computed, and every waveform
    is what its utterance gives alone, exact zeros past its end."""

    def __init__(self, model, vocoder, device=None, ragged=False):
        self.model, self.vocoder, self.ragged = model, vocoder, ragged
        self.device = torch.device(device) if device is not None else next(vocoder.parameters()).device
        self.acoustic_stream = torch.cuda.Stream(self.device)
        self._pending = collections.deque()

    def submit(self, *model_args, **model_kwargs):
        caller = torch.cuda.current_stream(self.device)
        self.acoustic_stream.wait_stream(caller)
        for a in (*model_args, *model_kwargs.values()):  # keyword tensors too: e_control / d_control as (B, T) tensors
            if torch.is_tensor(a) and a.is_cuda:
                a.record_stream(self.acoustic_stream)
        with torch.cuda.stream(self.acoustic_stream):
            out = self.model(*model_args, **model_kwargs)
            ev = torch.cuda.Event()
            ev.record(self.acoustic_stream)
        self._pending.append((out, ev))

    def pending(self):
        return len(self._pending)

    def next_wav(self):
        if not self._pending:
            raise RuntimeError("SynthesisPipeline.next_wav: nothing submitted")
        out, ev = self._pending.popleft()
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        for t in out:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(cur)
        # postnet mel is channels-last (B, T, 80): no transpose; out[9] (mel_len) was recorded on this stream above
        return out, self.vocoder.run(out[1], out[9] if self.ragged else None)


class SynthesisInputs:
    """The static input tensors of a ``GraphedSynthesis`` (``gs.inputs``): what the captured graph reads.  A call
    copies its arguments here (``GlyphBatch.to(device, n_chars=max_src_len)`` gives the ``images`` argument at this
    width).  ``widths`` (int32 (batch, max_src_len), pixels per character) exists with an ``atlas`` only: the graph's
    first launch then draws ``images`` from ``texts``, ``src_lens`` and ``widths``, so a replay follows a width
    changed in place here."""

    __slots__ = ("audiotypes", "texts", "src_lens", "images", "e_control", "d_control", "widths")

    def __init__(self, **tensors):
        for k in self.__slots__:
            setattr(self, k, tensors[k])


class SynthesisResult:
    """What a ``GraphedSynthesis`` call returns.  EVERY tensor here is owned by the captured graph: it is valid until
    the next call of the same ``GraphedSynthesis`` (which overwrites it in stream order) -- clone, or take ``wavs()``,
    before calling again.

    wav        (n, max_mel_len * hop): int16 with ``pcm_scale``, fp32 without; exactly 0 past each utterance's end.
               At the vocoder's rate (``rate``, 22050 Hz for the shipped HiFi-GAN); with ``out_rate`` at that rate,
               (n, resample_length(max_mel_len * hop, rate, out_rate))
    samples    (n,) int64: min(mel_len, max_mel_len) * hop, computed inside the graph; with ``out_rate`` the
               resampled counts, ceil(that M / O) (vo_resample's out_lens)
    mel_len    (n,) int64: the length regulator's uncropped frame counts
    truncated  (n,) bool: mel_len > max_mel_len -- the utterance was cropped at the capacity (as the reference's
               pad(output, max_len) crops it); re-run it in a larger bucket
    outputs    the model's 10-tuple (rows [:n])"""

    __slots__ = ("wav", "samples", "mel_len", "truncated", "outputs")

    def __init__(self, wav, samples, mel_len, truncated, outputs):
        self.wav, self.samples, self.mel_len, self.truncated, self.outputs = wav, samples, mel_len, truncated, outputs

    def wavs(self):
        """n numpy arrays, utterance i cut to its ``samples[i]``: one copy of ``wav`` and one of ``samples`` to the
        host (the arrays are views of that host copy, not of the graph's memory)."""
        wav = self.wav.cpu().numpy()
        samples = self.samples.cpu().numpy()
        return [wav[i, :int(samples[i])] for i in range(wav.shape[0])]


class GraphedSynthesis:
    """Glyph strips -> waveform (int16 PCM with ``pcm_scale``, e.g. 32768.0) as ONE captured graph per call:
    free-running ``model(...)`` with ``max_mel_len`` as the mel capacity, then the ragged
    ``vocoder.run(out[1], out[9], pcm_scale)`` on the model's own device-side ``mel_len`` -- no host read, no Python
    launch per kernel.  The shapes ``(batch, max_src_len, max_mel_len)`` are fixed for the object; a caller that wants
    several shape buckets keeps several objects.

    ``gs(audiotypes, src_lens, images, texts=None, e_control=None, d_control=None)`` takes n <= batch requests
    (device tensors, or host tensors / arrays, which are copied before the replay) and, on the current stream,
    copies them into the static inputs (``gs.inputs``), replays the graph and returns a ``SynthesisResult`` whose
    tensors the graph owns: VALID UNTIL THE NEXT CALL.  Rows n ... batch - 1 are filled with copies of request 0 and
    not reported.  Controls: whatever ``ops.control_view`` accepts for (n, max_src_len); ``None`` resets to 1.0.
    ``texts`` (the model reads only its shape under ``use_image``): ``None`` stores zeros.

    ``atlas`` (a ``dataset.GlyphAtlas`` already on the device, its ``cell``, ``stride`` and glyph height those of the
    model's glyph encoder: ValueError otherwise): the images are drawn inside the graph.  The captured body's first
    launch is ``vo_glyph_stretch`` from ``inputs.texts``, ``inputs.src_lens`` and ``inputs.widths`` into
    ``inputs.images``, and the call is ``gs(audiotypes, src_lens, texts=..., widths=None)``:
    ``texts`` (symbol ids) is required, ``images`` is refused, ``widths`` (n, max_src_len) are pixels per character
    (``None`` resets them to the glyphs' own width: unstretched).  Host arrays are validated as
    ``GlyphAtlas.layout`` validates them; device tensors are not read.  A replay follows ``inputs.widths`` changed in
    place and glyphs edited in place in ``atlas.glyphs_d``.  Without ``atlas`` nothing of this exists: the same
    arguments, the same graph.

    ``out_rate`` (delivery at another sample rate than the vocoder's ``rate``): the vocoder
    runs to fp32 and the captured body ends in one ``vo_resample`` launch from the fp32 waveform and ``samples``
    (cast to int32 inside the graph), which writes int16 with ``pcm_scale`` and fp32 without.  A ratio the library
    does not run is a ValueError here.  With ``out_rate=None`` (or equal to ``rate``) the object captures exactly
    the launches it captures without the argument.

    The model and the vocoder must be in eval mode (RuntimeError otherwise); the call runs under ``no_grad``.

    Capture: on a side stream after ``warmup`` eager runs (they build the weight packs, the vocoder's side streams
    and the allocator state), into a private memory pool.  The graph holds the ADDRESSES of the packed weights, so
    the capture remembers what ``HipModule._packed`` keys its caches on, for both modules -- parameter and buffer
    versions, compute dtypes, ``_pack_gen`` and the global generation -- and holds the pack objects themselves, so
    their memory outlives any rebuild.  When that key has moved (``load_state_dict``, ``set_precision``, an optimizer
    step, ``invalidate_packs``), a module has rebuilt its pack (a precision change and back with an eager run in
    between) or a submodule has been replaced, the next call captures again before it replays and ``gs.captures``
    goes up by one: a replay never synthesises with weights the modules no longer hold."""

    def __init__(self, model, vocoder, batch, max_src_len, max_mel_len, pcm_scale=None, use_image=True, warmup=2,
                 atlas=None, out_rate=None, rate=22050):
        from .train import _check_graph_runtime
        _check_graph_runtime("GraphedSynthesis (HIP-graph replay)")
        batch, max_src_len, max_mel_len = int(batch), int(max_src_len), int(max_mel_len)
        if batch < 1 or max_src_len < 1 or max_mel_len < 1:
            raise ValueError(f"GraphedSynthesis: batch, max_src_len and max_mel_len must be >= 1, got "
                             f"({batch}, {max_src_len}, {max_mel_len})")
        if max_mel_len > model.decoder.max_seq_len:
            # above it Decoder.run builds a sinusoid table on the host: not capturable
            raise ValueError(f"GraphedSynthesis: max_mel_len {max_mel_len} exceeds the model's max_seq_len "
                             f"{model.decoder.max_seq_len}")
        if max_src_len > model.encoder.max_seq_len:
            raise ValueError(f"GraphedSynthesis: max_src_len {max_src_len} exceeds the model's max_seq_len "
                             f"{model.encoder.max_seq_len}")
        if int(warmup) < 1:
            raise ValueError("GraphedSynthesis: warmup must be >= 1 (the weight packs are built by an eager run)")
        if pcm_scale is not None and not (0.0 < float(pcm_scale) < float("inf")):
            raise ValueError(f"GraphedSynthesis: pcm_scale must be finite and positive, got {pcm_scale}")
        self.model, self.vocoder = model, vocoder
        self.batch, self.max_src_len, self.max_mel_len = batch, max_src_len, max_mel_len
        self.pcm_scale = None if pcm_scale is None else float(pcm_scale)
        self.use_image, self.warmup = bool(use_image), int(warmup)
        self.rate = int(rate)
        self.out_rate = None if out_rate is None or int(out_rate) == self.rate else int(out_rate)
        if self.out_rate is not None:
            from . import ops
            ops.resample_geometry(self.rate, self.out_rate)  # ValueError for a ratio the library does not run
        self.device = next(vocoder.parameters()).device
        self.hop = 1
        for u in vocoder.h.upsample_rates:
            self.hop *= u
        dev = self.device
        images = None
        if self.use_image:
            vfe = model.encoder.VisualFeatureExtractor
            width = (max_src_len + 2 * (vfe.stride // 2)) * vfe.slice_width  # n_chars * cell + 2 * margin
            images = torch.ones((batch, vfe.dim3, vfe.slice_height, width), dtype=torch.float32, device=dev)
        self.atlas, widths = atlas, None
        if atlas is not None:
            if not self.use_image:
                raise ValueError("GraphedSynthesis: atlas draws the images: it needs use_image=True")
            if atlas.glyphs_d is None or atlas.glyphs_d.device != dev:
                raise ValueError(f"GraphedSynthesis: atlas must be on the vocoder's device {dev} (atlas.to(device)), "
                                 f"it is on {atlas.device}")
            have = (atlas.cell, atlas.stride, atlas.height, 1)
            want = (vfe.slice_width, vfe.stride, vfe.slice_height, vfe.dim3)
            if have != want:
                raise ValueError(f"GraphedSynthesis: atlas (cell, stride, height, channels) = {have} does not match "
                                 f"the model's glyph encoder {want}")
            widths = torch.full((batch, max_src_len), atlas.src_w, dtype=torch.int32, device=dev)
        self.inputs = SynthesisInputs(
            widths=widths,
            audiotypes=torch.zeros(batch, dtype=torch.int64, device=dev),
            texts=torch.zeros((batch, max_src_len), dtype=torch.int64, device=dev),
            src_lens=torch.full((batch,), max_src_len, dtype=torch.int64, device=dev),
            images=images,
            e_control=torch.ones((batch, max_src_len), dtype=torch.float32, device=dev),
            d_control=torch.ones((batch, max_src_len), dtype=torch.float32, device=dev))
        self._side = torch.cuda.Stream(dev)
        self.graph = self._out = self._state = None
        self._texts_set = False
        self._modules = []
        self.captures = 0

    # ------------------------------------------------------------------ capture

    def _weights_state(self):
        """(key, packs, children) of both modules, through the module list of the last capture.
        key: what ``HipModule._packed`` keys the packed-weight caches on -- the versions of every parameter and buffer
        (looked up through their modules, so one replaced inside its module is seen), every HIP module's compute
        dtype and ``_pack_gen``, the global generation.
        packs: every HIP module's cached pack object itself.  A module keeps ONE pack, so a change there and back
        (``set_precision`` to fp32, an eager run, back to mixed) brings the key back while the pack the graph reads
        was dropped and rebuilt: the capture HOLDS these objects, which keeps the graph's addresses valid, and a call
        compares them by identity.
        children: every module's child objects, by identity: a submodule swapped for another."""
        from ._base import _GENERATION, HipModule
        key = [_GENERATION[0], getattr(self.model, "stream_dtype", None)]
        packs, children = [], []
        for m in self._modules:
            for t in m._parameters.values():
                key.append(None if t is None else t._version)
            for t in m._buffers.values():
                key.append(None if t is None else t._version)
            children.extend(m._modules.values())
            if isinstance(m, HipModule):
                key.append(m.compute_dtype)
                key.append(m.__dict__.get("_pack_gen", 0))
                cache = m.__dict__.get("_pack_cache")
                packs.append(cache.get("val") if cache else None)
        return key, packs, children

    def _stale(self):
        """True when the graph must be captured (again) before it may replay."""
        if self.graph is None:
            return True
        key, packs, children = self._weights_state()
        k0, p0, c0 = self._state
        return (key != k0 or len(packs) != len(p0) or len(children) != len(c0)
                or any(a is not b for a, b in zip(packs, p0)) or any(a is not b for a, b in zip(children, c0)))

    def _body(self):
        i = self.inputs
        if self.atlas is not None:  # every element of i.images is written
            from . import ops
            a = self.atlas
            ops.glyph_stretch(a.glyphs_d, a.table_d, i.texts, i.src_lens, i.widths, a.cell, a.margin,
                              W_out=i.images.shape[3], out=i.images)
        out = self.model(i.audiotypes, i.texts, i.src_lens, self.max_src_len, None, None, self.max_mel_len, None,
                         None, None, i.images, None, self.use_image, e_control=i.e_control, d_control=i.d_control)
        mel_len = out[9]
        samples = torch.clamp(mel_len, max=self.max_mel_len) * self.hop
        if self.out_rate is None:
            wav = self.vocoder.run(out[1], out[9], self.pcm_scale)
        else:
            from . import ops
            wav, samples = ops.resample(self.vocoder.run(out[1], out[9], None), self.rate, self.out_rate,
                                        lens=samples.to(torch.int32), pcm_scale=self.pcm_scale)
            samples = samples.to(torch.int64)
        return out, wav, samples, mel_len > self.max_mel_len

    def _capture(self):
        cur = torch.cuda.current_stream(self.device)
        self.graph = self._out = self._state = None  # a re-capture releases the old graph's pool and packs first
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            for _ in range(self.warmup):
                self._body()
        cur.wait_stream(self._side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self._side):  # no pool given: a private one
            out = self._body()
        self.graph, self._out = graph, out
        self._modules = [m for root in (self.model, self.vocoder) for m in root.modules()]
        self._state = self._weights_state()  # after the runs: they built the packs it describes, and holds them
        self.captures += 1

    # ------------------------------------------------------------------ call

    def _checked(self, dst, src, n, name):
        src = torch.as_tensor(src)
        if tuple(src.shape) != tuple(dst[:n].shape):
            raise ValueError(f"GraphedSynthesis: {name} must have shape {tuple(dst[:n].shape)} "
                             f"(n = {n} requests of this object's bucket), got {tuple(src.shape)}")
        return dst, src

    def _fill(self, dst, src, n):
        dst[:n].copy_(src, non_blocking=True)
        if n < self.batch:  # rows n ... batch - 1: copies of request 0
            dst[n:].copy_(dst[:1].expand(self.batch - n, *dst.shape[1:]))

    def __call__(self, audiotypes, src_lens, images=None, texts=None, e_control=None, d_control=None, widths=None):
        from . import ops
        if self.model.training or self.vocoder.training:
            raise RuntimeError("GraphedSynthesis: the model and the vocoder must be in eval mode")
        src_lens = torch.as_tensor(src_lens)
        n = src_lens.shape[0] if src_lens.dim() == 1 else 0
        if not 1 <= n <= self.batch:
            raise ValueError(f"GraphedSynthesis: src_lens must have shape (n,) with 1 <= n <= batch = {self.batch}, "
                             f"got {tuple(src_lens.shape)}")
        i = self.inputs
        atlas = self.atlas
        if atlas is not None:
            if images is not None:
                raise ValueError("GraphedSynthesis: this object draws its images from an atlas inside the graph: pass "
                                 "texts (and widths), not images")
            if texts is None:
                raise ValueError(f"GraphedSynthesis: an atlas needs texts (symbol ids) of shape "
                                 f"{tuple(i.texts[:n].shape)}")
            texts, widths = atlas.on_device(texts, widths)  # host arrays: validated; device tensors: not read
        elif widths is not None:
            raise ValueError("GraphedSynthesis: widths need an atlas (GraphedSynthesis(..., atlas=...)); this object "
                             "takes images")
        elif self.use_image and images is None:
            raise ValueError(f"GraphedSynthesis: use_image needs images of shape {tuple(i.images[:n].shape)}")
        if not self.use_image and texts is None:
            raise ValueError(f"GraphedSynthesis: use_image=False needs texts of shape {tuple(i.texts[:n].shape)}")
        # every argument is checked before the first copy: a refused call leaves the static inputs as they were
        copies = [self._checked(i.audiotypes, audiotypes, n, "audiotypes"),
                  self._checked(i.src_lens, src_lens, n, "src_lens")]
        if self.use_image and atlas is None:
            copies.append(self._checked(i.images, images, n, "images"))
        if texts is not None:
            copies.append(self._checked(i.texts, texts, n, "texts"))
        if widths is not None:
            copies.append(self._checked(i.widths, widths, n, "widths"))
        with torch.no_grad(), torch.cuda.device(self.device):
            for dst, control in ((i.e_control, e_control), (i.d_control, d_control)):
                if control is not None:  # converted to fp32 on the device where it is not (ops.control_view)
                    c = ops.control_view(control, n, self.max_src_len, device=self.device)[0]
                    copies.append((dst, c.expand(n, self.max_src_len)))
            for dst, src in copies:
                self._fill(dst, src, n)
            if texts is None and self._texts_set:  # no texts: zeros (PAD), not what an earlier call left
                i.texts.zero_()
            self._texts_set = texts is not None
            for dst, control in ((i.e_control, e_control), (i.d_control, d_control)):
                if control is None:
                    dst.fill_(1.0)
            if atlas is not None and widths is None:  # unstretched, not what an earlier call left
                i.widths.fill_(atlas.src_w)
            if self._stale():
                self._capture()
            self.graph.replay()
        out, wav, samples, truncated = self._out
        outputs = tuple(t[:n] if torch.is_tensor(t) else t for t in out)
        return SynthesisResult(wav[:n], samples[:n], outputs[9], truncated[:n], outputs)
