"""Golden vectors for the glyph encoder's config surface (context stride, conv kernel sizes, layer count,
BatchNorm / bridge ReLU on or off), from the reference itself.

Runs only where the reference is mounted (see make_goldens.py, whose ``import_reference`` this reuses).
Written, as data only:

    vfe_cfg_<name>.npz   the reference's VisualFeatureExtractor class instantiated directly at slice_height 8,
                         slice_width 10, embed_dim 32, eval(): every parameter and buffer (``sd.<key>``), random
                         images (2, 1, 8, 10 * (5 + stride - 1)), ``out``, and the configuration (stride, kernel,
                         layers, embed_normalize, bridge_relu).  Parameters are drawn here (seeded); the BatchNorm
                         running statistics are drawn too, not left at 0 / 1.
    vtts_tf_s3.npz       the ten outputs of the teacher-forced vTTS forward with visual_text.stride = 3 on
                         vtts_tf's inputs, the images padded by 102 columns of 1.0 on each side as
                         pad_2D_gray_image does (inputs not repeated).
    vtts_s3_spec.json    vtts_spec.json with the one shape stride 3 changes: bridge.0.weight (256, 7344).

    python tests/golden/make_goldens_vfe.py
"""

import copy
import json
import os

import numpy as np

import make_goldens as MG

NAMES = ["mel", "postnet_mel", "e_pred", "k_pred", "log_d_pred", "d_rounded",
         "src_masks", "mel_masks", "src_lens_out", "mel_lens_out"]
H, SW, EMBED, CHARS = 8, 10, 32, 5
# name, stride, kernel, layers, embed_normalize, bridge_relu
CASES = (("s3_k33_l3", 3, (3, 3), 3, True, True),
         ("s1_k53_l2", 1, (5, 3), 2, True, True),
         ("s2_k35_l1", 2, (3, 5), 1, True, True),
         ("s3_k11_l4", 3, (1, 1), 4, False, False))
BRIDGE_KEY = "encoder.VisualFeatureExtractor.bridge.0.weight"


def draw_parameters(module, rng):
    """Taps U(-0.5, 0.5), conv bias and BatchNorm shift positive, BatchNorm scale near 1, running statistics
    drawn: the ReLU stack stays alive (checked by the caller).  Bridge: U(+-1/sqrt(fan_in))."""
    import torch
    sd = module.state_dict()
    convs = {k.rsplit(".", 1)[0] for k, v in sd.items() if v.dim() == 4}
    with torch.no_grad():
        for k, v in sd.items():
            mod, leaf = k.rsplit(".", 1)
            if leaf == "num_batches_tracked":
                continue
            if mod in convs:
                a = rng.uniform(-0.5, 0.5, size=v.shape) if leaf == "weight" else rng.uniform(0.2, 0.6, size=v.shape)
            elif k.startswith("embedder."):
                a = {"weight": rng.uniform(0.7, 1.3, size=v.shape), "bias": rng.uniform(0.1, 0.5, size=v.shape),
                     "running_mean": rng.uniform(-0.3, 0.3, size=v.shape),
                     "running_var": rng.uniform(0.5, 1.5, size=v.shape)}[leaf]
            else:
                bound = 1.0 / np.sqrt(sd[mod + ".weight"].shape[1])
                a = rng.uniform(-bound, bound, size=v.shape)
            v.copy_(torch.from_numpy(a.astype(np.float32)))


def module_cases():
    import torch
    from model.visual_feature_extractor import VisualFeatureExtractor
    for idx, (name, stride, kernel, layers, norm, relu) in enumerate(CASES):
        rng = np.random.default_rng(9100 + idx)
        m = VisualFeatureExtractor("gray-scale", SW, H, EMBED, stride, embed_normalize=norm, bridge_relu=relu,
                                   kernel_size=kernel, num_convolutions=layers)
        draw_parameters(m, rng)
        m.eval()
        images = rng.uniform(0.0, 1.0, size=(2, 1, H, SW * (CHARS + stride - 1))).astype(np.float32)
        with torch.no_grad():
            out = m(torch.from_numpy(images))
            n = out.shape[1]
            win = torch.from_numpy(images).unfold(3, SW * stride, SW)[:, :, :, :n]
            emb = m.embedder(win.permute(0, 3, 1, 2, 4).reshape(2 * n, 1, H, SW * stride).contiguous())
        alive = float((emb > 0).float().mean())
        assert alive >= 0.25, (name, alive)
        MG.save("vfe_cfg_" + name, images=images, out=MG.t2n(out), stride=np.int64(stride),
                kernel=np.array(kernel, np.int64), layers=np.int64(layers), embed_normalize=np.bool_(norm),
                bridge_relu=np.bool_(relu), **{"sd." + k: MG.t2n(v) for k, v in m.state_dict().items()})
        print(name, "out", tuple(out.shape), "alive", round(alive, 3))


def whole_model(cfg):
    import torch
    from model import vTTS
    with open(os.path.join(MG.HERE, "vtts_spec.json")) as f:
        committed = json.load(f)
    expect = [[k, [256, 7344] if k == BRIDGE_KEY else s, t] for k, s, t in committed["spec"]]
    assert sum(k == BRIDGE_KEY for k, _, _ in expect) == 1
    pc = copy.deepcopy(cfg["preprocess"])
    pc["visual_text"]["stride"] = 3
    torch.manual_seed(0)
    model = vTTS(pc, cfg["model"], cfg["train"])
    spec = MG.spec_of(model.state_dict())
    assert json.loads(json.dumps(spec)) == expect, "stride 3 changes more than bridge.0.weight"
    with open(os.path.join(MG.HERE, "vtts_s3_spec.json"), "w") as f:
        json.dump({"seed": committed["seed"], "spec": spec}, f)
    MG.load_into(model, MG.make_state_dict(spec, MG.VTTS_SEED))
    model.eval()
    tf = np.load(os.path.join(MG.HERE, "vtts_tf.npz"))
    tb = {k[3:]: tf[k] for k in tf.files if k.startswith("in_")}
    tb["images"] = np.pad(tb["images"], [(0, 0), (0, 0), (0, 0), (102, 102)], mode="constant", constant_values=1.0)
    tt = {k: (torch.from_numpy(v) if v.ndim else v.item()) for k, v in tb.items()}
    with torch.no_grad():
        out = model(tt["audiotypes"], tt["texts"], tt["src_lens"], tt["max_src_len"], tt["mels"], tt["mel_lens"],
                    tt["max_mel_len"], tt["e_targets"], None, tt["d_targets"], tt["images"], None, True)
    MG.save("vtts_tf_s3", **{n: MG.t2n(o) for n, o in zip(NAMES, out) if o is not None})


def main():
    cfg = MG.import_reference()
    module_cases()
    whole_model(cfg)


if __name__ == "__main__":
    main()
