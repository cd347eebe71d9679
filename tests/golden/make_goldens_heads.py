"""Golden vectors for attention head counts 4 and 8 (d_k = 64 and 32 at hidden 256), from the reference itself.

Runs only where the reference is mounted (see make_goldens.py, whose ``import_reference`` this reuses).  The
reference's vTTS is built with ``encoder_head = decoder_head = H`` for H in (4, 8): its state dict has the keys
and shapes of vtts_spec.json (n_head * d_k = 256 either way), so the committed deterministic weights and the
committed ``vtts_tf`` inputs are reused unchanged.  Written, as data only:

    vtts_tf_h{H}.npz   the ten outputs of the teacher-forced forward on vtts_tf's inputs (inputs not repeated)
    fft_dec_h{H}.npz   decoder FFT block 0 at L = 64, lens [64, 41]: x, lens, out, attn (as fft_dec)

    python tests/golden/make_goldens_heads.py
"""

import copy
import json
import os

import numpy as np

import make_goldens as MG

NAMES = ["mel", "postnet_mel", "e_pred", "k_pred", "log_d_pred", "d_rounded",
         "src_masks", "mel_masks", "src_lens_out", "mel_lens_out"]
HEADS = (4, 8)


def main():
    cfg = MG.import_reference()
    import torch
    from model import vTTS
    from utils.tools import get_mask_from_lengths

    with open(os.path.join(MG.HERE, "vtts_spec.json")) as f:
        committed = json.load(f)
    tf = np.load(os.path.join(MG.HERE, "vtts_tf.npz"))
    tb = {k[3:]: tf[k] for k in tf.files if k.startswith("in_")}
    tt = {k: (torch.from_numpy(v) if v.ndim else v.item()) for k, v in tb.items()}
    for H in HEADS:
        mc = copy.deepcopy(cfg["model"])
        mc["transformer"]["encoder_head"] = H
        mc["transformer"]["decoder_head"] = H
        torch.manual_seed(0)
        model = vTTS(cfg["preprocess"], mc, cfg["train"])
        spec = MG.spec_of(model.state_dict())
        assert json.loads(json.dumps(spec)) == committed["spec"], "the state-dict spec depends on the head count"
        MG.load_into(model, MG.make_state_dict(spec, MG.VTTS_SEED))
        model.eval()
        with torch.no_grad():
            out = model(tt["audiotypes"], tt["texts"], tt["src_lens"], tt["max_src_len"], tt["mels"], tt["mel_lens"],
                        tt["max_mel_len"], tt["e_targets"], None, tt["d_targets"], tt["images"], None, True)
            MG.save(f"vtts_tf_h{H}", **{n: MG.t2n(o) for n, o in zip(NAMES, out) if o is not None})
            rng = np.random.default_rng(700 + H)
            L, lens = 64, [64, 41]
            x = rng.normal(0, 1, size=(2, L, 256)).astype(np.float32)
            mask = get_mask_from_lengths(torch.tensor(lens), L)
            y, attn = model.decoder.layer_stack[0](torch.from_numpy(x), mask=mask,
                                                   slf_attn_mask=mask.unsqueeze(1).expand(-1, L, -1))
            MG.save(f"fft_dec_h{H}", x=x, lens=np.array(lens), out=MG.t2n(y), attn=MG.t2n(attn))


if __name__ == "__main__":
    main()
