"""Training / evaluation dataset with the glyph layout on the GPU (SURVEY.md 8(f) row 2;
reference: scripts/dataset.py:13-202, scripts/utils/tools.py:22-72,585-635,
scripts/04_train.py:47-58).

Same constructor, ``__getitem__`` keys, ``collate_fn`` (sort by text length, split the
batch_size x group_size loader batch into batch_size groups, optional tail) and 13-item
batch tuple as the reference.  What moves: the reference centres every character of the
rendered strip into a ``max_pixelsize``-wide white cell with cv2/numpy per sample in the
DataLoader workers, pads the batch with ``pad_2D_gray_image`` and converts with
``ToTensor`` on the host.  Here a sample carries its raw strip and per-character widths;
``reprocess`` puts them in a :class:`GlyphBatch`, and ``utils.tools.to_device`` lays the
whole batch out on the GPU in one ``vo_glyph_batch`` launch -- the host does no per-pixel
work, which is what keeps 8 data-parallel ranks fed.  PNG decoding uses PIL (cv2 is not a
dependency of this package).
"""

import json
from pathlib import Path

import numpy as np
from torch.utils.data import Dataset as _TorchDataset

from .utils.symbols import get_symbols
from .utils.tools import pad_1D, pad_2D


class GlyphBatch:
    """Raw grayscale strips (H, W_b) uint8 and their per-character widths for one batch.
    ``to(device)`` -> (B, 1, H, W) fp32 laid out exactly as the reference's
    character_padding_forinput + pad_2D_gray_image + ToTensor (bit-identical)."""

    def __init__(self, strips, char_widths, cell, stride):
        self.strips = [np.ascontiguousarray(s, dtype=np.uint8) for s in strips]
        self.char_widths = [np.asarray(w, np.int64).reshape(-1) for w in char_widths]
        self.cell, self.stride = int(cell), int(stride)

    def __len__(self):
        return len(self.strips)

    @property
    def margin(self):
        return (self.stride // 2) * self.cell  # pad_2D_gray_image's each_padlen

    def to(self, device, n_chars=None):
        """``n_chars``: lay the batch out at the width of an ``n_chars``-character bucket, ``n_chars * cell +
        2 * margin`` (the static image tensor of ``pipeline.GraphedSynthesis``); the columns past the batch's own
        width are white (1.0)."""
        from . import ops
        W_out = None
        if n_chars is not None:
            longest = max((len(w) for w in self.char_widths), default=0)
            if int(n_chars) < longest:
                raise ValueError(f"GlyphBatch.to: n_chars={n_chars} is below the batch's longest text ({longest})")
            W_out = int(n_chars) * self.cell + 2 * self.margin
        return ops.glyph_batch(self.strips, self.char_widths, self.cell, self.margin, device, W_out=W_out)


def widths_from_rates(rates, fontsize):
    """Per-character pixel widths from the user's stretch rates, as prediction.ipynb computes them
    (``int(fs * im_w_rate)``: a float64 product truncated toward zero), elementwise -> int32 array."""
    r = np.asarray(rates, np.float64)
    return np.array([int(fontsize * float(v)) for v in r.reshape(-1)], np.int32).reshape(r.shape)


def allocate_widths(n_chars, canvas_width):
    """The widths the training renderer gives the characters of an ``n_chars``-character text on a canvas
    ``canvas_width`` pixels wide (``Generator._canvas_allocate``, visualtext_generator.py:19-21) -> int32 (n_chars,)."""
    n_chars, canvas_width = int(n_chars), int(canvas_width)
    return np.array([(canvas_width + i) // n_chars for i in range(n_chars)]).astype(np.int32)


class GlyphAtlas:
    """The unstretched glyphs of the vocabulary, ``glyphs`` (n_symbols, H, S) uint8 indexed by symbol id (row 0: PAD),
    and what lays a batch of texts out from them on the GPU with a pixel width per character: the resize of the
    reference's renderers (``c_im.resize((width, fontsize))``, PIL's bicubic, bit-exact) and ``GlyphBatch``'s
    layout in one launch that reads ids, lengths and widths on the device (``ops.glyph_stretch``, DESIGN.md section
    13).  Font rasterisation stays with the caller (``render`` does it with PIL).

    ``to(device)`` uploads the glyphs and the coefficient table once and keeps them (``.glyphs_d``, ``.table_d``);
    ``glyphs_d`` edited in place is what the next launch, or graph replay, reads."""

    def __init__(self, glyphs, cell, stride=1):
        glyphs = np.ascontiguousarray(glyphs)
        if glyphs.dtype != np.uint8 or glyphs.ndim != 3 or 0 in glyphs.shape:
            raise ValueError(f"GlyphAtlas: glyphs must be uint8 (n_symbols, H, S), got {glyphs.dtype} {glyphs.shape}")
        self.glyphs = glyphs
        self.cell, self.stride = int(cell), int(stride)
        if self.cell < 1 or self.stride < 1:
            raise ValueError(f"GlyphAtlas: cell and stride must be >= 1, got ({cell}, {stride})")
        self.device = self.glyphs_d = self.table_d = None

    n_symbols = property(lambda self: self.glyphs.shape[0])
    height = property(lambda self: self.glyphs.shape[1])
    src_w = property(lambda self: self.glyphs.shape[2])

    @property
    def margin(self):
        return (self.stride // 2) * self.cell  # as GlyphBatch.margin

    def to(self, device):
        import torch
        from . import ops
        self.device = torch.device(device)
        self.glyphs_d = torch.from_numpy(self.glyphs).to(self.device)
        self.table_d = torch.from_numpy(ops.glyph_stretch_table(self.src_w, self.cell)).to(self.device)
        return self

    def _ints(self, a, name, dtype, lo, hi, what):
        """A host sequence validated and uploaded, or a device tensor taken as it is (never read here)."""
        import torch
        if torch.is_tensor(a) and a.is_cuda:
            return a
        h = np.asarray(a.cpu() if torch.is_tensor(a) else a)
        if h.dtype.kind not in "iu":
            raise ValueError(f"GlyphAtlas: {name} must be integers, got {h.dtype}")
        if lo is not None and h.size and (int(h.min()) < lo or int(h.max()) > hi):
            raise ValueError(f"GlyphAtlas: {name} must be in [{lo}, {hi}] ({what}), got "
                             f"[{int(h.min())}, {int(h.max())}]")
        return torch.from_numpy(np.ascontiguousarray(h, dtype)).to(self.device, non_blocking=True)

    def on_device(self, texts, widths=None):
        """(texts int64, widths int32 or None) on the atlas's device.  Host sequences are validated (ValueError for
        an id outside the atlas or a width outside [0, cell]) and uploaded; device tensors are returned as they
        are, unread: the kernel whitens what is out of range there."""
        if self.glyphs_d is None:
            raise RuntimeError("GlyphAtlas: call to(device) first")
        ids = self._ints(texts, "texts", np.int64, 0, self.n_symbols - 1, "the atlas's symbol ids")
        w = None if widths is None else self._ints(widths, "widths", np.int32, 0, self.cell, "0 to the cell width")
        return ids, w

    def layout(self, texts, src_lens, widths=None, n_chars=None, out=None):
        """``texts`` (B, T) symbol ids, ``src_lens`` (B,), ``widths`` (B, T) pixels (None: the glyphs unstretched) ->
        (B, 1, H, n_chars * cell + 2 * margin) fp32 on the atlas's device (``n_chars``: T unless given; the columns
        past T characters are white): what ``GlyphBatch.to(device, n_chars)`` gives for the strips of the same
        characters at the same widths.  Host sequences are validated and uploaded, device tensors (int64, int64,
        int32) are not read on the host (``on_device``): there an id outside the atlas or a width <= 0 is a white
        cell, and a width above the cell is the cell."""
        from . import ops
        ids, w = self.on_device(texts, widths)
        lens = self._ints(src_lens, "src_lens", np.int64, None, None, None)
        if ids.dim() != 2:
            raise ValueError(f"GlyphAtlas.layout: texts must have shape (B, T), got {tuple(ids.shape)}")
        T = ids.shape[1]
        n_chars = T if n_chars is None else int(n_chars)
        if n_chars < T:
            raise ValueError(f"GlyphAtlas.layout: n_chars={n_chars} is below the texts' length ({T})")
        return ops.glyph_stretch(self.glyphs_d, self.table_d, ids, lens, w, self.cell, self.margin,
                                 W_out=n_chars * self.cell + 2 * self.margin, out=out)

    @classmethod
    def render(cls, symbols, font, fontsize, background=(255, 255, 255), text=(0, 0, 0), cell=None, stride=1):
        """Draw the atlas with PIL as the reference draws a character (visualtext_generator.py:36-38:
        ``Image.new("RGB", (fs, fs), bg)``, ``draw.text((0, 0), ch, fill, font)``; ``convert("L")`` as its loaders
        do).  ``symbols``: {character: id} (``utils.symbols.get_symbols``) or a sequence of characters (ids from 1);
        id 0 (PAD) and ids without a character are background.  ``font``: a path (loaded at ``fontsize``) or a PIL
        font object.  The colours must be gray: the reference resizes the three channels separately, which is the
        resize of L only when they are equal."""
        from PIL import Image, ImageDraw, ImageFont
        background, text = tuple(int(v) for v in background), tuple(int(v) for v in text)
        for name, col in (("background", background), ("text", text)):
            if len(col) != 3 or len(set(col)) != 1 or not 0 <= col[0] <= 255:
                raise ValueError(f"GlyphAtlas.render: {name} colour {col} is not gray (three equal values in 0..255)")
        if not isinstance(symbols, dict):
            symbols = {s: i + 1 for i, s in enumerate(symbols)}
        if any(int(i) < 1 for i in symbols.values()):
            raise ValueError("GlyphAtlas.render: symbol ids start at 1 (0 is PAD)")
        fs = int(fontsize)
        if isinstance(font, (str, bytes)) or hasattr(font, "__fspath__"):
            font = ImageFont.truetype(str(font), fs)
        glyphs = np.full((max(symbols.values(), default=0) + 1, fs, fs), background[0], np.uint8)
        for ch, i in symbols.items():
            c_im = Image.new("RGB", (fs, fs), background)
            ImageDraw.Draw(c_im).text((0, 0), ch, fill=text, font=font)
            glyphs[int(i)] = np.asarray(c_im.convert("L"), dtype=np.uint8)
        return cls(glyphs, fs if cell is None else cell, stride)

    @classmethod
    def from_config(cls, preprocess_config, font=None):
        """The atlas of a preprocess config: ``visual_text.fontsize / color / stride``, the font at ``path.font``
        (or ``font``), the vocabulary and ``visual_text.json``'s max_pixelsize of ``path.preprocessed``."""
        vt = preprocess_config["visual_text"]
        pre = Path(preprocess_config["path"]["preprocessed"])
        with open(pre / "visual_text.json") as f:
            cell = json.load(f)["max_pixelsize"][0]
        return cls.render(get_symbols(pre), preprocess_config["path"]["font"] if font is None else font,
                          vt["fontsize"], vt["color"]["background"], vt["color"]["text"], cell, vt["stride"])


def _read_gray(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("L"), dtype=np.uint8)


class Dataset(_TorchDataset):
    def __init__(self, filename, preprocess_config, train_config, model_config, sort=False, drop_last=False):
        self.preprocessed_path = Path(preprocess_config["path"]["preprocessed"])
        self.batch_size = train_config["optimizer"]["batch_size"]
        self.input_type = preprocess_config["input_type"]
        self.symbol_to_id = get_symbols(self.preprocessed_path)
        self.sort = sort
        self.drop_last = drop_last
        self.use_image = train_config["use_image"]
        self.is_energy = model_config["variance_embedding"]["is_energy_condition"]
        self.is_kurtosis = model_config["variance_embedding"]["is_kurtosis_condition"]
        if self.input_type == "visual-text":
            vt = preprocess_config["visual_text"]
            self.text_font_size = vt["fontsize"]
            self.image_bgcolor = vt["color"]["background"]
            self.image_textcolor = vt["color"]["text"]
            self.image_loadscale = vt["scale_in_training"]
            if self.image_loadscale != "gray-scale":
                raise NotImplementedError("RGB glyph input: the reference's pad_2D_image path is not on the "
                                          "ICASSP configuration")
            with open(self.preprocessed_path / "visual_text.json") as f:
                info = json.load(f)
            self.width = info["max_pixelsize"][0]
            self.height = info["height"][0]
            self.stride = vt["stride"]
        self.basename, self.audiotype, self.fontsize, self.fonttype, self.text = self.process_meta(filename)
        with open(self.preprocessed_path / "audiotype.json") as f:
            self.audiotype_map = json.load(f)

    def __len__(self):
        return len(self.text)

    def __getitem__(self, idx):
        basename = self.basename[idx]
        audiotype = self.audiotype[idx]
        tmp_text = self.text[idx].replace("{", "").replace("}", "").replace("\n", "")
        text = np.array([self.symbol_to_id[t] for t in list(tmp_text)])
        p = self.preprocessed_path
        mel = np.load(p / "mel" / audiotype / f"{basename}.npy")
        energy = np.load(p / "energy" / audiotype / f"{basename}.npy") if self.is_energy else None
        kurtosis = np.load(p / "kurtosis" / audiotype / f"{basename}.npy") if self.is_kurtosis else None
        duration = np.load(p / "duration" / audiotype / f"{basename}.npy")
        image = None
        if self.use_image:
            widths = np.load(p / "image" / "width" / audiotype / f"{basename}.npy").astype(np.int32)
            if np.max(widths) > self.width:
                print(f"image length is over {self.width} pixels. {basename}")
            image = (_read_gray(p / "image" / "png" / audiotype / f"{basename}.png"), widths)
        return {"id": basename, "audiotype": self.audiotype_map[audiotype], "text": text, "mel": mel,
                "energy": energy, "kurtosis": kurtosis, "duration": duration, "image": image,
                "event_image_feature": None}

    def process_meta(self, filename):
        names, audiotypes, fonttypes, fontsizes, texts = [], [], [], [], []
        with open(self.preprocessed_path / filename, "r", encoding="utf-8") as f:
            for line in f.readlines():
                fn, at, fs, ft, r = line.strip("\n").split("|")
                names.append(fn)
                audiotypes.append(at)
                fonttypes.append(ft)
                fontsizes.append(fs)
                texts.append(r)
        return names, audiotypes, fonttypes, fontsizes, texts

    def reprocess(self, data, idxs):
        ids = [data[i]["id"] for i in idxs]
        audiotypes = np.array([data[i]["audiotype"] for i in idxs])
        texts = [data[i]["text"] for i in idxs]
        mels = [data[i]["mel"] for i in idxs]
        energies = [data[i]["energy"] for i in idxs]
        kurtosises = [data[i]["kurtosis"] for i in idxs]
        durations = [data[i]["duration"] for i in idxs]
        text_lens = np.array([t.shape[0] for t in texts])
        mel_lens = np.array([m.shape[0] for m in mels])
        texts = pad_1D(texts)
        mels = pad_2D(mels)
        energies = pad_1D(energies) if energies[0] is not None else None
        kurtosises = pad_1D(kurtosises) if kurtosises[0] is not None else None
        durations = pad_1D(durations)
        images = None
        if self.use_image:
            images = GlyphBatch([data[i]["image"][0] for i in idxs], [data[i]["image"][1] for i in idxs],
                                self.width, self.stride)
        event_image_features = np.array([data[i]["event_image_feature"] for i in idxs])
        return (ids, audiotypes, texts, text_lens, max(text_lens), mels, mel_lens, max(mel_lens), energies,
                kurtosises, durations, images, event_image_features)

    def collate_fn(self, data):
        n = len(data)
        if self.sort:
            idx_arr = np.argsort(-np.array([d["text"].shape[0] for d in data]))
        else:
            idx_arr = np.arange(n)
        tail = idx_arr[len(idx_arr) - (len(idx_arr) % self.batch_size):]
        idx_arr = idx_arr[: len(idx_arr) - (len(idx_arr) % self.batch_size)]
        idx_arr = idx_arr.reshape((-1, self.batch_size)).tolist()
        if not self.drop_last and len(tail) > 0:
            idx_arr += [tail.tolist()]
        return [self.reprocess(data, idx) for idx in idx_arr]


class DeviceCorpus:
    """The base utterances packed once on the GPU, and training batches assembled from them by a *plan* in one launch
    (``vo_augment_batch``): the repeat and consecutive augmentations of the reference
    (scripts/preprocessor/preprocessor.py:468-622), ``pad_1D`` / ``pad_2D`` and ``GlyphBatch``'s layout, without a file
    or a host copy per variant.  A plan row is ``src, pos, m, m_mel, r`` (``preprocessor.augment``); ``batch`` returns
    the 13-item tuple ``utils.tools.to_device(Dataset.reprocess(...))`` returns, element for element."""

    def __init__(self):
        raise TypeError("DeviceCorpus: use from_arrays or from_dataset")

    @classmethod
    def from_arrays(cls, utterances, cell, stride, device):
        """``utterances``: a list of dicts with the keys ``Dataset.__getitem__`` returns (id, audiotype, text, mel,
        energy, kurtosis, duration, image = (strip, widths)); energy / kurtosis None for all or for none."""
        import torch
        from . import _lib
        self = object.__new__(cls)
        self.cell, self.stride, self.device = int(cell), int(stride), torch.device(device)
        if self.cell < 1 or self.stride < 1:
            raise ValueError(f"DeviceCorpus: cell and stride must be >= 1, got ({cell}, {stride})")
        if not utterances:
            raise ValueError("DeviceCorpus: no utterances")
        self.names, self.texts, self.durations = [], [], []
        flat = {k: [] for k in ("id", "dur", "dstart", "width", "col", "energy", "kurtosis", "mel", "px")}
        strip_w, audiotype = [], []
        has = {k: utterances[0][k] is not None for k in ("energy", "kurtosis")}
        n_mels = H = None
        for i, u in enumerate(utterances):
            who = f"DeviceCorpus: utterance {i} ({u.get('id')!r})"
            text, dur = np.asarray(u["text"]).reshape(-1), np.asarray(u["duration"]).reshape(-1)
            mel = np.asarray(u["mel"])
            if u.get("image") is None:
                raise ValueError(f"{who}: has no image (a Dataset with use_image)")
            strip, width = np.asarray(u["image"][0]), np.asarray(u["image"][1]).reshape(-1)
            n = len(text)
            per_char = {"duration": dur, "widths": width}
            for k in ("energy", "kurtosis"):
                if (u[k] is not None) != has[k]:
                    raise ValueError(f"{who}: {k} is given for some utterances and None for others")
                if has[k]:
                    per_char[k] = np.asarray(u[k]).reshape(-1)
            if n < 1 or any(len(a) != n for a in per_char.values()):
                raise ValueError(f"{who}: the text has {n} characters, "
                                 + ", ".join(f"{k} {len(a)}" for k, a in per_char.items()) + " (all equal and >= 1)")
            if dur.dtype.kind not in "iu" or width.dtype.kind not in "iu" or int(dur.min()) < 0 or int(width.min()) < 0:
                raise ValueError(f"{who}: durations and widths must be integers >= 0")
            if mel.ndim != 2 or mel.shape[0] != int(dur.sum()):
                raise ValueError(f"{who}: the mel has shape {mel.shape}, the durations sum to {int(dur.sum())} frames")
            if strip.ndim != 2 or strip.dtype != np.uint8 or strip.shape[1] != int(width.sum()):
                raise ValueError(f"{who}: the strip is {strip.dtype} {strip.shape}, the widths sum to "
                                 f"{int(width.sum())} columns (a gray uint8 (H, sum widths) strip)")
            n_mels, H = n_mels or mel.shape[1], H or strip.shape[0]
            if mel.shape[1] != n_mels or strip.shape[0] != H or min(n_mels, H) < 1:
                raise ValueError(f"{who}: {mel.shape[1]} mel bins and {strip.shape[0]} strip rows, the corpus has "
                                 f"{n_mels} and {H}")
            self.names.append(u.get("id"))
            self.texts.append(tuple(int(t) for t in text))
            self.durations.append(dur.astype(np.int64))
            audiotype.append(int(u["audiotype"]))
            strip_w.append(strip.shape[1])
            flat["id"].append(text)
            flat["dur"].append(dur)
            flat["dstart"].append(np.cumsum(dur) - dur)
            flat["width"].append(width)
            flat["col"].append(np.cumsum(width) - width)
            flat["mel"].append(mel.astype(np.float32, copy=False))
            flat["px"].append(strip.reshape(-1))
            for k in ("energy", "kurtosis"):
                if has[k]:
                    flat[k].append(per_char[k].astype(np.float32))  # as to_device's .float()
        self.n_chars = [len(t) for t in self.texts]
        self.n_frames = [int(d.sum()) for d in self.durations]
        self.n_mels, self.height = int(n_mels), int(H)
        off = lambda sizes: np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])  # noqa: E731
        host = {"char_off": off(self.n_chars).astype(np.int32), "frame_off": off(self.n_frames).astype(np.int64),
                "px_off": off([H * w for w in strip_w])[:-1].astype(np.int64), "strip_w": np.asarray(strip_w, np.int32),
                "audiotype": np.asarray(audiotype, np.int64), "mel": np.concatenate(flat["mel"]),
                "px": np.concatenate(flat["px"])}
        if int(host["frame_off"][-1]) * self.n_mels >= 2 ** 62 or int(off(self.n_chars)[-1]) >= 2 ** 31:
            raise ValueError("DeviceCorpus: too large")
        for k in ("id", "dur", "dstart", "width", "col"):
            host["ch_" + k] = np.concatenate(flat[k]).astype(np.int32)
        for k in ("energy", "kurtosis"):
            host["ch_" + k] = np.concatenate(flat[k]) if has[k] else None
        # the device arrays live as long as the corpus: the struct holds their addresses
        self.tensors = {k: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
                        for k, a in host.items()}
        self.struct = _lib.Corpus(U=len(self.texts), n_mels=self.n_mels, strip_h=self.height,
                                  **{k: None if t is None else t.data_ptr() for k, t in self.tensors.items()})
        self.last_status = None
        self.normalized = False
        self.waves = None
        return self

    def attach_waves(self, wavs, hop, max_wav_value=32768.0, sr=None, target_sr=None, start=None):
        """The base utterances' waveforms beside their mels, for the vocoder's training batches
        (``hifigan.data.SegmentSampler``): ``wavs`` is one 1-D array per utterance in corpus
        order, all int16 (PCM as the files hold it, kept as int16 and divided by ``max_wav_value`` when a segment is
        cut) or all floating point (kept as fp32, copied as they are).  Packed once, flat, every utterance at a sample
        offset that is a multiple of 8.  ``hop``: the hop of the corpus's mels; utterance u of N samples and F frames
        must have 1 + N // hop >= F, what ``FeatureExtractor.process`` requires of a waveform and its durations.
        ValueError naming the utterance otherwise.  Sets ``self.waves`` (``_lib.WaveCorpus``) and returns self.

        ``sr`` (an int, or one per utterance): the rate the arrays are at, with ``target_sr`` the rate of the corpus's
        mels.  Where the two differ the waveforms are resampled on the device (``ops.resample``, one launch per source
        rate) and the corpus holds fp32, whatever came in; ``start`` (seconds, one per
        utterance) drops the first ``int(target_sr * start)`` resampled samples, as ``FeatureExtractor.process``
        does.  The frame check then uses the resampled, trimmed length.  Without ``sr`` the call is what it was."""
        import torch
        from . import _lib
        if sr is None and (target_sr is not None or start is not None):
            raise ValueError("DeviceCorpus.attach_waves: target_sr and start go with sr, the rate of the arrays")
        if sr is not None and target_sr is None:
            raise ValueError("DeviceCorpus.attach_waves: sr needs target_sr, the rate of the corpus's mels")
        hop, max_wav_value = int(hop), float(max_wav_value)
        if hop < 1:
            raise ValueError(f"DeviceCorpus.attach_waves: hop must be >= 1, got {hop}")
        if not (np.isfinite(max_wav_value) and max_wav_value > 0):
            raise ValueError(f"DeviceCorpus.attach_waves: max_wav_value must be finite and > 0, got {max_wav_value}")
        wavs = list(wavs)
        if len(wavs) != len(self):
            raise ValueError(f"DeviceCorpus.attach_waves: {len(wavs)} waveforms for {len(self)} utterances")
        arrays, is_int16 = [], None
        for i, a in enumerate(wavs):
            who = f"DeviceCorpus.attach_waves: utterance {i} ({self.names[i]!r})"
            a = np.asarray(a.cpu() if torch.is_tensor(a) else a)
            if a.ndim != 1 or a.size < 1:
                raise ValueError(f"{who}: the waveform has shape {a.shape} (1-D and non-empty)")
            if a.dtype != np.int16 and a.dtype.kind != "f":
                raise ValueError(f"{who}: the waveform is {a.dtype} (int16 or floating point)")
            if is_int16 is None:
                is_int16 = a.dtype == np.int16
            if (a.dtype == np.int16) != is_int16:
                raise ValueError(f"{who}: the waveform is {a.dtype}, the ones before it are "
                                 f"{'int16' if is_int16 else 'floating point'} (all int16 or all floating point)")
            arrays.append(a)
        if sr is not None:
            arrays = self._resampled(arrays, is_int16, max_wav_value, sr, int(target_sr), start)
            is_int16 = is_int16 and not torch.is_tensor(arrays[0])
        for i, a in enumerate(arrays):
            size = a.numel() if torch.is_tensor(a) else a.size
            if size < 1 or 1 + size // hop < self.n_frames[i]:
                raise ValueError(f"DeviceCorpus.attach_waves: utterance {i} ({self.names[i]!r}): {size} samples are "
                                 f"1 + N // hop = {1 + size // hop} frames at hop {hop}, the mel has "
                                 f"{self.n_frames[i]}")
        dtype = np.int16 if is_int16 else np.float32
        n = np.asarray([a.numel() if torch.is_tensor(a) else a.size for a in arrays], np.int64)
        off = np.concatenate([[0], np.cumsum((n + 7) // 8 * 8)]).astype(np.int64)
        if torch.is_tensor(arrays[0]):  # resampled: fp32 rows on the device already
            flat = torch.zeros(int(off[-1]), dtype=torch.float32, device=self.device)
            for a, o in zip(arrays, off):
                flat[o:o + a.numel()] = a
        else:
            flat = np.zeros(int(off[-1]), dtype)
            for a, o in zip(arrays, off):
                flat[o:o + a.size] = a
            flat = torch.from_numpy(flat).to(self.device)
        self.n_samples = [int(v) for v in n]
        self.wave_hop = hop
        self.wave_tensors = {"sample_off": torch.from_numpy(off).to(self.device),
                             "n_samples": torch.from_numpy(n).to(self.device), "wav": flat}
        self.waves = _lib.WaveCorpus(U=len(self), is_int16=int(is_int16), max_wav_value=max_wav_value,
                                     **{k: t.data_ptr() for k, t in self.wave_tensors.items()})
        return self

    def _resampled(self, arrays, is_int16, max_wav_value, sr, target_sr, start):
        """``attach_waves`` with ``sr``: the validated host arrays -> one fp32 device row per utterance at
        ``target_sr``, or the arrays themselves when every rate already is ``target_sr`` and nothing is trimmed.  The
        lengths are computed on the host (``ops.resample_len``): nothing is read back."""
        import torch
        from . import ops
        U = len(arrays)
        rates = [int(sr)] * U if np.ndim(sr) == 0 else [int(r) for r in sr]
        starts = [0.0] * U if start is None else [float(v) for v in start]
        if len(rates) != U or len(starts) != U:
            raise ValueError(f"DeviceCorpus.attach_waves: {U} utterances, {len(rates)} rates, {len(starts)} start "
                             "times")
        if any(not (v >= 0.0 and v < float("inf")) for v in starts):
            raise ValueError(f"DeviceCorpus.attach_waves: start times must be finite and >= 0, got {starts}")
        skips = [int(target_sr * v) for v in starts]
        if all(r == target_sr for r in rates) and not any(skips):
            return arrays
        geo = {r: ops.resample_geometry(r, target_sr) for r in set(rates) - {target_sr}}  # refusals first
        rows = [None] * U
        for rate in sorted(set(rates)):
            idx = [i for i, r in enumerate(rates) if r == rate]
            if rate == target_sr:  # trimmed on the host, read as the kernel reads them
                for i in idx:
                    a = arrays[i][skips[i]:]
                    a = a.astype(np.float32) / np.float32(max_wav_value) if is_int16 else a.astype(np.float32)
                    rows[i] = torch.from_numpy(a).to(self.device)
                continue
            x = np.zeros((len(idx), max(arrays[i].size for i in idx)), np.int16 if is_int16 else np.float32)
            for k, i in enumerate(idx):
                x[k, :arrays[i].size] = arrays[i]
            y, _ = ops.resample(torch.from_numpy(x).to(self.device), rate, target_sr,
                                lens=[arrays[i].size for i in idx], skip=[skips[i] for i in idx],
                                max_wav_value=max_wav_value if is_int16 else None)
            for k, i in enumerate(idx):
                L = max(ops.resample_len(arrays[i].size, *geo[rate][:2]) - skips[i], 0)
                rows[i] = y[k, :L]
        return rows

    @classmethod
    def from_dataset(cls, ds, indices=None, base_only=True, device="cuda"):
        """The samples ``indices`` (all by default) of a ``Dataset``, each read once through ``ds[i]``.  ``base_only``:
        names that carry an augmentation suffix (a metadata file that already lists the reference's variants) are
        left out."""
        from .preprocessor.augment import is_variant_name
        idx = range(len(ds)) if indices is None else indices
        return cls.from_arrays([ds[i] for i in idx if not (base_only and is_variant_name(ds.basename[i]))],
                               ds.width, ds.stride, device)

    def __len__(self):
        return len(self.texts)

    @property
    def margin(self):
        return (self.stride // 2) * self.cell  # as GlyphBatch.margin

    def variants(self, cfg, mel_copies="reference"):
        """(names, plan int32 (N, 5)) of the whole augmented corpus: for every utterance its base row and then the
        variants ``preprocessor.augment.variants`` lists, named as the reference saves them.  An epoch is a shuffle of
        row indices."""
        from .preprocessor import augment as AU
        names, rows = [], []
        for u, text in enumerate(self.texts):
            for suffix, pos, m, mm, r, _ in [("", 0, 0, 0, 1, text)] + AU.variants(text, cfg, mel_copies):
                names.append(f"{self.names[u]}{suffix}")
                rows.append((u, pos, m, mm, r))
        return names, np.asarray(rows, np.int32)

    def _stats_plan(self, plan, cfg):
        """The plan of ``stats`` / ``normalize_`` on the device: a device tensor as it is (never read back), a host plan
        through ``check_plan``'s range rules without caps, None -> ``variants(cfg)`` or the base rows."""
        import torch
        from .preprocessor import augment as AU
        if torch.is_tensor(plan) and plan.is_cuda:
            return plan
        if plan is None:
            plan = self.variants(cfg)[1] if cfg is not None else [(u, 0, 0, 0, 1) for u in range(len(self))]
        p, _, _ = AU.check_plan(plan.numpy() if torch.is_tensor(plan) else plan, self.n_chars, self.n_frames,
                                self.durations)
        return torch.from_numpy(p).to(self.device, non_blocking=True)

    def _stats_device(self, plan_d):
        """feature -> the (6,) float64 ``out`` of ``ops.corpus_stats`` on the device, for the features the corpus has."""
        from . import ops
        outs = {}
        for k in ("energy", "kurtosis"):
            if self.tensors["ch_" + k] is not None:
                outs[k], self.last_status = ops.corpus_stats(self.struct, plan_d, k)
        if not outs:
            raise ValueError("DeviceCorpus: the corpus was packed without energy and kurtosis")
        return outs

    @staticmethod
    def _stats_host(outs):
        """``stats.json``'s [min, max, mean, std] per feature: one device-to-host copy each."""
        res = {}
        for k, o in outs.items():
            _, mean, std, lo, hi, _ = (np.float64(v) for v in o.cpu().numpy())
            if lo > hi:
                raise ValueError(f"DeviceCorpus: no plan row was accepted for the {k} statistics (last_status has the "
                                 "reasons)")
            res[k] = [float((lo - mean) / std), float((hi - mean) / std), float(mean), float(std)]
        return res

    def stats(self, plan=None, cfg=None):
        """``stats.json`` of the corpus augmented by ``plan`` -> {"energy": [min, max, mean, std], "kurtosis": [...]}
        (the features the corpus has), as the reference's ``build_from_path`` computes them over every file it wrote
        (scripts/preprocessor/preprocessor.py:113-144): per row the interquartile outlier rule,
        mean and population std over what all rows keep, min and max of the normalised values of every character.  No
        variant is materialised.  ``plan``: rows ``src, pos, m, m_mel, r``; None: ``variants(cfg)[1]`` with ``cfg``
        (the ``augmentation:`` block), the base utterances alone without.  A host plan is checked first (ValueError
        naming the row); a device plan is never read back.  A row longer than ``_lib.STATS_MAX_CHARS`` characters is
        refused on the device and contributes nothing: ``self.last_status`` has the rows' codes.  On a corpus that
        ``normalize_`` has already normalised these are the statistics of the normalised values."""
        return self._stats_host(self._stats_device(self._stats_plan(plan, cfg)))

    def normalize_(self, stats=None, plan=None, cfg=None):
        """Z-normalise ``ch_energy`` / ``ch_kurtosis`` in place, ``(x - mean) / std`` in float64 rounded to float32 (the
        reference's ``_normalize`` followed by ``to_device``'s ``.float()``), and return the stats dict.  ``stats``:
        that of ``stats()`` or a ``stats.json``; None: computed from ``plan`` / ``cfg`` as ``stats`` does, and then mean
        and std go from the statistics kernel to the normalising one on the device.  ``batch`` afterwards gives the
        normalised values.  A second call raises ValueError: normalising twice is silent corruption."""
        import torch
        from . import ops
        if self.normalized:
            raise ValueError("DeviceCorpus.normalize_: the corpus is already normalised")
        have = [k for k in ("energy", "kurtosis") if self.tensors["ch_" + k] is not None]
        if stats is None:
            outs = self._stats_device(self._stats_plan(plan, cfg))
            stats = self._stats_host(outs)  # before anything is written: raises when no row was accepted
        else:
            if plan is not None or cfg is not None:
                raise ValueError("DeviceCorpus.normalize_: give stats, or plan / cfg to compute them, not both")
            outs = {}
            for k in have:
                if k not in stats or len(stats[k]) != 4:
                    raise ValueError(f"DeviceCorpus.normalize_: stats has no [min, max, mean, std] for {k}")
                mean, std = float(stats[k][2]), float(stats[k][3])
                if not (np.isfinite(mean) and np.isfinite(std) and std > 0):
                    raise ValueError(f"DeviceCorpus.normalize_: {k} mean {mean}, std {std} (finite, std > 0)")
                outs[k] = torch.tensor([0.0, mean, std, 0.0, 0.0, 0.0], dtype=torch.float64).to(self.device)
            stats = {k: [float(v) for v in stats[k]] for k in have}
        for k in have:
            ops.corpus_normalize_(self.tensors["ch_" + k], outs[k])
        self.normalized = True
        return stats

    def batch(self, plan, max_src_len=None, max_mel_len=None, out=None, names=None):
        """The batch of ``plan`` -> (ids, audiotypes, texts, src_lens, max_src_len, mels, mel_lens, max_mel_len,
        energies, kurtosises, durations, images, None) on the corpus's device, with ``to_device``'s dtypes.

        ``plan`` on the host (numpy or a sequence of rows) is checked first: a row out of range or over a cap is a
        ValueError naming the row and the rule, and nothing is launched.  Without caps the caps are the batch's own
        maxima, as ``Dataset.reprocess`` pads.  ``ids`` are the reference's save names (or ``names``).
        ``plan`` as an int32 (B, 5) tensor on the device is never read back: the caps are required, ``ids`` is
        ``names`` (None by default), and a bad row comes out as an empty utterance with its reason in
        ``self.last_status`` (``_lib.AUG_*``).  ``out``: the tuple of an earlier call of the same shapes, refilled in
        place (a static batch for a captured training step)."""
        import torch
        from . import ops
        from .preprocessor import augment as AU
        if torch.is_tensor(plan) and plan.is_cuda:
            if max_src_len is None or max_mel_len is None:
                raise ValueError("DeviceCorpus.batch: a device plan needs max_src_len and max_mel_len")
            plan_d, ids = plan, names
        else:
            p, src_lens, mel_lens = AU.check_plan(plan.numpy() if torch.is_tensor(plan) else plan, self.n_chars,
                                                  self.n_frames, self.durations, max_src_len, max_mel_len)
            max_src_len = max(src_lens) if max_src_len is None else max_src_len
            max_mel_len = max(max(mel_lens), 1) if max_mel_len is None else max_mel_len
            ids = names if names is not None else [
                f"{self.names[s]}{AU.suffix_of(self.texts[s], pos, m, r)}" for s, pos, m, _, r in p.tolist()]
            plan_d = torch.from_numpy(p).to(self.device, non_blocking=True)
        max_src_len, max_mel_len = int(max_src_len), int(max_mel_len)
        if names is not None and len(names) != plan_d.shape[0]:
            raise ValueError(f"DeviceCorpus.batch: {len(names)} names for {plan_d.shape[0]} plan rows")
        o = None
        if out is not None:
            o = dict(zip(("audiotypes", "texts", "src_lens", "mels", "mel_lens", "energies", "kurtosises", "durations",
                          "images"), [out[i] for i in (1, 2, 3, 5, 6, 8, 9, 10, 11)]))
            st = self.last_status
            if st is None or st.shape[0] != plan_d.shape[0]:
                st = torch.empty(plan_d.shape[0], dtype=torch.int32, device=self.device)
            o["status"] = st
        o = ops.augment_batch(self.struct, plan_d, max_src_len, max_mel_len, self.height, self.cell, self.margin, out=o)
        self.last_status = o["status"]
        return (ids, o["audiotypes"], o["texts"], o["src_lens"], max_src_len, o["mels"], o["mel_lens"], max_mel_len,
                o["energies"], o["kurtosises"], o["durations"], o["images"], None)
