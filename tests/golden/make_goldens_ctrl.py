"""Golden vectors for tensor-valued energy / duration controls, from the reference itself.

Runs only where the reference is mounted (see make_goldens.py, whose ``import_reference`` this reuses).  The
reference's ``vTTS.forward`` takes ``e_control`` / ``d_control`` as (B, T) tensors (scripts/model/vtts.py:68-69) and
broadcasts them against its (B, T_src) predictions (scripts/model/modules.py:59,111).  On the ``vtts_inf`` recipe
(``synth.acoustic_batch(123, 2, 5, 20, ragged=True)``, duration bias shifted by DUR_BIAS_SHIFT) this writes, as data
only, inputs + controls + the ten outputs:

    vtts_inf_ctrl_tok.npz   per-token controls (2, 5): e_control ~ U[0.5, 1.6], d_control ~ U[0, 2.5] with one exact
                            0.0 and one exact 1.0 planted
    vtts_inf_ctrl_utt.npz   per-utterance controls (2, 1), same distributions

Both discontinuous steps are kept away from their edges so that a last-ulp difference cannot flip them: on the
reference's own values, for every unmasked token, exp(log_d) - 1 is at least D_MARGIN from a half-integer and the
controlled, re-normalised energy is at least E_MARGIN from the nearest bin edge (about 1/50 of the 0.0243 bin
width).  Both are asserted and the margins met are stored in the archives; a control draw that misses moves on to the
next seed, the margins stay.

    python tests/golden/make_goldens_ctrl.py
"""

import numpy as np

import make_goldens as MG

NAMES = ["mel", "postnet_mel", "e_pred", "k_pred", "log_d_pred", "d_rounded",
         "src_masks", "mel_masks", "src_lens_out", "mel_lens_out"]
D_MARGIN, E_MARGIN = 5e-3, 5e-4
FIRST_SEED, MAX_SEEDS = 7, 64
PLANT = {"tok": (((0, 1), 0.0), ((1, 2), 1.0)), "utt": ()}  # exact d_control values at unmasked tokens


def draw(seed, shape, plant):
    rng = np.random.default_rng(seed)
    ec = rng.uniform(0.5, 1.6, size=shape).astype(np.float32)
    dc = rng.uniform(0.0, 2.5, size=shape).astype(np.float32)
    for pos, v in plant:
        dc[pos] = v
    return ec, dc


def margins(log_d, e_pred, bins, valid):
    """(duration margin, energy margin) over the unmasked tokens, in float64 of the reference's fp32 values."""
    r = np.exp(log_d.astype(np.float64)) - 1.0
    d_m = np.abs(r - (np.floor(r) + 0.5))[valid].min()
    e_m = np.abs(e_pred.astype(np.float64)[..., None] - bins.astype(np.float64)).min(-1)[valid].min()
    return float(d_m), float(e_m)


def main():
    cfg = MG.import_reference()
    import torch
    torch.manual_seed(0)
    from model import vTTS
    from visual_onoma_to_wave_amd import synth

    model = vTTS(cfg["preprocess"], cfg["model"], cfg["train"])
    MG.load_into(model, MG.make_state_dict(MG.spec_of(model.state_dict()), MG.VTTS_SEED))
    model.eval()
    bins = MG.t2n(model.variance_adaptor.energy_bins)
    b = synth.acoustic_batch(123, 2, 5, 20, ragged=True)
    tb = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in b.items()}
    with torch.no_grad():
        model.variance_adaptor.duration_predictor.linear_layer.bias += MG.DUR_BIAS_SHIFT
        for tag, shape in (("tok", (2, 5)), ("utt", (2, 1))):
            for seed in range(FIRST_SEED, FIRST_SEED + MAX_SEEDS):
                ec, dc = draw(seed, shape, PLANT[tag])
                out = model(tb["audiotypes"], tb["texts"], tb["src_lens"], tb["max_src_len"],
                            None, None, None, None, None, None, tb["images"], None, True,
                            e_control=torch.from_numpy(ec), d_control=torch.from_numpy(dc))
                res = {n: MG.t2n(o) for n, o in zip(NAMES, out) if o is not None}
                d_m, e_m = margins(res["log_d_pred"], res["e_pred"], bins, ~res["src_masks"])
                print(f"{tag}: control seed {seed}: duration margin {d_m:.3e}, energy margin {e_m:.3e}")
                if d_m >= D_MARGIN and e_m >= E_MARGIN:
                    break
            assert d_m >= D_MARGIN and e_m >= E_MARGIN, (tag, d_m, e_m)
            assert res["e_pred"].dtype == np.float32 and res["d_rounded"].dtype == np.float32
            MG.save("vtts_inf_ctrl_" + tag, **{"in_" + k: np.asarray(v) for k, v in b.items()},
                    e_control=ec, d_control=dc, control_seed=np.int64(seed),
                    dur_bias_shift=np.float32(MG.DUR_BIAS_SHIFT), d_margin=np.float64(d_m),
                    e_margin=np.float64(e_m), **res)


if __name__ == "__main__":
    main()
