"""Which augmented variants of a base utterance exist (reference: scripts/preprocessor/preprocessor.py:468-501,
597-622), as plan rows for ``dataset.DeviceCorpus``.  Host only: no file is written, the
variants themselves are assembled on the GPU by ``vo_augment_batch``.

A variant is ``(suffix, pos, m, m_mel, r, text_out)``: ``m`` more copies of character ``pos``, ``m_mel`` more copies
of its mel frames, the whole repeated ``r`` times.  The base is ``("", 0, 0, 0, 1, text)``.
"""

import re

import numpy as np

MEL_COPIES = ("reference", "durations")
_VARIANT = re.compile(r"-(repeat\d+|(first)?consecutive\d+(-repeat\d+)?)$")


def consecutive_pos(text):
    """``Preprocessor._get_consecutive_pos``: the middle (rounded down) of the first run of three or more equal
    characters, or None.  ``text``: a string or any sequence of comparable items (symbol ids).  Only the first
    such run counts, whatever follows it; the golden pins the answers (tests/golden/augment.npz)."""
    pre = None  # the reference starts from "", which no character equals
    s_i, cnt = -1, 1
    for i, ch in enumerate(text):
        if pre is not None and ch == pre:
            s_i = i - 1 if cnt == 1 else s_i
            cnt += 1
        else:
            if cnt >= 3:
                return s_i + int((i - 1 - s_i) / 2)
            s_i, cnt, pre = -1, 1, ch
    if cnt >= 3:
        return s_i + int((len(text) - 1 - s_i) / 2)
    return None


def _seq(text):
    return text if isinstance(text, (str, list, tuple)) else tuple(np.asarray(text).reshape(-1).tolist())


def _mel_copies(m, mel_copies):
    if mel_copies not in MEL_COPIES:
        raise ValueError(f"mel_copies must be one of {MEL_COPIES}, got {mel_copies!r}")
    return m + 1 if (mel_copies == "reference" and m > 0) else m


def variants(text, cfg, mel_copies="reference"):
    """The variants ``Preprocessor._augmentation`` writes for one base ``text``, in its order, as
    ``[(suffix, pos, m, m_mel, r, text_out), ...]`` (the base itself is not in the list).  ``cfg``: the
    ``augmentation:`` block of preprocess.yaml.  ``mel_copies``: "reference" gives a consecutive variant the mel the
    reference's files have, one copy of the character's frames more than its durations say (m_mel = m + 1);
    "durations" gives m_mel = m."""
    text = _seq(text)
    max_len, rep_n = int(cfg["max_length"]), int(cfg["repeat_num"])
    cons_n, first_n = int(cfg["consecutive_num"]), int(cfg["first_consecutive"])
    out = []
    if len(text) <= max_len:
        for r in range(2, rep_n + 1):
            out.append((f"-repeat{r}", 0, 0, 0, r, text * r))

        def consecutive(pos, m):
            return text[:pos] + text[pos:pos + 1] * (m + 1) + text[pos + 1:]

        for k in range(1, first_n + 1):
            out.append((f"-firstconsecutive{k}", 0, k, _mel_copies(k, mel_copies), 1, consecutive(0, k)))
        pos = consecutive_pos(text)
        if pos is not None:
            for k in range(1, cons_n + 1):
                t = consecutive(pos, k)
                mm = _mel_copies(k, mel_copies)
                out.append((f"-consecutive{k}", pos, k, mm, 1, t))
                if len(t) <= max_len:  # the nested repeats test the augmented text
                    for r in range(2, rep_n + 1):
                        out.append((f"-consecutive{k}-repeat{r}", pos, k, mm, r, t * r))
    return out


def is_variant_name(name):
    """Whether a metadata name carries one of the suffixes ``variants`` gives (a file the reference's augmentation
    wrote, not a base utterance)."""
    return _VARIANT.search(name) is not None


def suffix_of(text, pos, m, r):
    """The reference's suffix of plan row ``(pos, m, ., r)`` on base ``text``: ``-consecutive{m}`` at the text's
    ``consecutive_pos``, ``-firstconsecutive{m}`` at 0 otherwise, then ``-repeat{r}``.  A position the reference never
    augments is named ``-pos{pos}consecutive{m}``."""
    s = ""
    if m > 0:
        if pos == consecutive_pos(_seq(text)):
            s = f"-consecutive{m}"
        else:
            s = f"-firstconsecutive{m}" if pos == 0 else f"-pos{pos}consecutive{m}"
    return s + (f"-repeat{r}" if r > 1 else "")


def out_sizes(n_chars, n_frames, d_pos, m, m_mel, r):
    """(characters, frames) of a plan row's output: (n + m) r and (F + m_mel d[pos]) r."""
    return (int(n_chars) + int(m)) * int(r), (int(n_frames) + int(m_mel) * int(d_pos)) * int(r)


def check_plan(plan, n_chars, n_frames, durations, max_src_len=None, max_mel_len=None):
    """Validate a host plan by the rules the device refuses a row by (include/vonoma.h) -> (plan int32 (B, 5),
    src_lens, mel_lens).  ``n_chars`` / ``n_frames``: per base utterance; ``durations``: list of per-character
    duration arrays.  ValueError names the row and the rule."""
    p = np.asarray(plan)
    if p.ndim != 2 or p.shape[1] != 5 or p.shape[0] < 1 or p.dtype.kind not in "iu":
        raise ValueError(f"plan must be integers of shape (B, 5) with B >= 1, got {p.dtype} {p.shape}")
    src_lens, mel_lens = [], []
    for b, (src, pos, m, mm, r) in enumerate(p.tolist()):
        row = f"plan row {b} (src {src}, pos {pos}, m {m}, m_mel {mm}, r {r})"
        if not 0 <= src < len(n_chars):
            raise ValueError(f"{row}: src is outside [0, {len(n_chars)})")
        if not 0 <= pos < n_chars[src]:
            raise ValueError(f"{row}: pos is outside [0, {n_chars[src]})")
        if m < 0 or mm < 0 or r < 1:
            raise ValueError(f"{row}: m and m_mel must be >= 0 and r >= 1")
        L, FL = out_sizes(n_chars[src], n_frames[src], durations[src][pos], m, mm, r)
        if max_src_len is not None and L > max_src_len:
            raise ValueError(f"{row}: {L} characters are over max_src_len = {max_src_len}")
        if max_mel_len is not None and FL > max_mel_len:
            raise ValueError(f"{row}: {FL} frames are over max_mel_len = {max_mel_len}")
        src_lens.append(L)
        mel_lens.append(FL)
    if int(np.abs(p).max()) >= 2 ** 31:
        raise ValueError("plan values do not fit int32")
    return np.ascontiguousarray(p, np.int32), src_lens, mel_lens
