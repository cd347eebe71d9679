"""The vocoder's receptive field, and the batch-dependence it causes in a padded batch.

The dense Generator computes every padded frame of a batch.  vTTS fills those frames with 0.0, and a log-mel of 0
is not silence, so the frames past an utterance's end reach its last frames through every conv's halo: the tail of
an utterance depends on what it was batched with.  The reference has the same artefact.  ``Generator.run(mel,
lengths)`` removes it by treating utterance b as a tensor of lengths[b] frames at every layer.

This CPU test pins the size of that tail on the oracle: R mel frames, the receptive field per side that DESIGN.md
section 10 counts (13.3 frames, R = 14 whole frames).  The GPU tests of the ragged generator hold the last R frames of
every utterance to their own error bar (tests/test_gpu_ragged_generator.py): a masking error of one row sits there.
"""

import numpy as np
import torch

from helpers import hifigan_arrays, hifigan_h

R_FRAMES = 14  # ceil(13.3)
HOP = 256


def _wavs():
    from oracle import vocoder as V
    torch.set_num_threads(8)
    gsd = V.fold_weight_norm({k: torch.from_numpy(np.array(v)) for k, v in hifigan_arrays().items()})
    g = torch.Generator().manual_seed(20)
    mel = torch.randn(2, 80, 40, generator=g) * 1.5 - 4.0
    mel[1, :, 20:] = 0.0  # utterance 1 is 20 frames long: padded as vTTS pads
    with torch.no_grad():
        batch = V.generator(gsd, mel, hifigan_h()).reshape(2, -1)
        alone = V.generator(gsd, mel[1:2, :, :20].contiguous(), hifigan_h()).reshape(-1)
    return batch[1, :20 * HOP].double().numpy(), alone.double().numpy()


def test_padded_batch_changes_only_the_last_R_frames():
    """Utterance 1 (20 of the batch's 40 frames) in the padded batch against the same utterance alone: equal to
    fp32 noise before sample 256 * (20 - R), different after it.  R is the structural bound; with these weights the
    outermost taps' contributions fall under fp32 noise, and the first sample that measurably differs (printed) lies
    about 8 frames before the end."""
    batch, alone = _wavs()
    assert batch.shape == alone.shape == (20 * HOP,)
    edge = HOP * (20 - R_FRAMES)
    diff = np.abs(batch - alone)
    scale = np.abs(alone).max()
    noise = 1e-5 * scale  # fp32 noise of a different batch size: other oneDNN blocking, same arithmetic
    print(f"max |diff| before sample {edge}: {diff[:edge].max():.3e}; after: {diff[edge:].max():.3e}; "
          f"signal peak {scale:.3e}")
    assert diff[:edge].max() <= noise
    assert diff[edge:].max() > 1e-2 * scale  # the artefact is real: percent of the signal's peak, not noise
    first = int(np.argmax(diff > noise))
    print(f"first differing sample {first} = frame {first / HOP:.2f} ({20 - first / HOP:.2f} frames before the end)")
    assert first >= edge
