"""Visual-glyph encoder front (reference: scripts/model/visual_feature_extractor.py:5-83).

The strip (B, 1, 24, 102*T) is cut into T character slices by the kernel grid itself
(no Python slicing loop, no stacked copies); each slice runs 3 x [Conv2d 3x3 (1 -> 1
channel) -> BatchNorm2d(eval) -> ReLU] in LDS (``vo_vfe_stencil``), then the bridge
Linear(2448 -> 256) + ReLU runs as a K=1 MFMA conv over all B*T slices at once.

That is the ICASSP configuration.  Every other gray-scale configuration of the reference's
configs -- ``visual_text.stride`` s >= 1 (slice i is the context window of cells i .. i+s-1
of the margin-padded strip), odd ``conv_kernel_size`` up to 9 x 9, any ``layer_num``,
``embed_normalize`` / ``bridge_relu`` on or off -- runs through ``vo_vfe_stencil_ex`` (one
workgroup per window, the whole window in LDS) and the same bridge.
"""

import torch
import torch.nn as nn

from .. import ops
from .._base import HipModule, fold_bn


class VisualFeatureExtractor(HipModule):
    def __init__(self, load_scale, slice_width, slice_height, embed_dim, stride, embed_normalize=True,
                 bridge_relu=True, kernel_size=(3, 3), num_convolutions=1):
        super().__init__()
        self.load_scale = load_scale
        self.dim3 = {"gray-scale": 1, "RGB-scale": 3}[load_scale]
        self.slice_width, self.slice_height = slice_width, slice_height
        self.embed_dim, self.stride = embed_dim, stride
        self.embed_normalize, self.bridge_relu = embed_normalize, bridge_relu
        kh, kw = kernel_size
        self.kernel_size = (slice_height, kw) if kh == -1 else (kh, kw)
        if self.kernel_size[0] % 2 == 0 or self.kernel_size[1] % 2 == 0:
            raise AssertionError(f"conv2d kernel {self.kernel_size} must be odd in both dims")
        self.num_convolutions = num_convolutions
        layers = []
        for _ in range(num_convolutions):
            layers.append(nn.Conv2d(self.dim3, self.dim3, kernel_size=self.kernel_size, stride=1,
                                    padding=((kh - 1) // 2, (kw - 1) // 2)))
            if embed_normalize:
                layers.append(nn.BatchNorm2d(self.dim3))
            layers.append(nn.ReLU(inplace=True))
        self.embedder = nn.Sequential(*layers)
        lin = nn.Linear(slice_width * stride * slice_height * self.dim3, embed_dim)
        self.bridge = nn.Sequential(lin, nn.ReLU(inplace=True)) if bridge_relu else lin
        for p in self.parameters():
            nn.init.uniform_(p, -0.08, 0.08)

    @property
    def _linear(self):
        return self.bridge[0] if self.bridge_relu else self.bridge

    def _icassp(self):
        """Stride 1, 3 x 3, BatchNorm, bridge ReLU: the configuration ``vo_vfe_stencil`` was written for."""
        return self.stride == 1 and self.kernel_size == (3, 3) and self.embed_normalize and self.bridge_relu

    def _supported(self):
        kh, kw = self.kernel_size
        H, win_w = self.slice_height, self.slice_width * self.stride
        if self.dim3 != 1:
            raise NotImplementedError("the HIP VFE covers gray-scale glyphs only (scale_in_training: RGB-scale is not "
                                      "supported)")
        if self.stride < 1 or self.num_convolutions < 1:
            raise NotImplementedError(f"the HIP VFE needs stride >= 1 and layer_num >= 1, got {self.stride} and "
                                      f"{self.num_convolutions}")
        if min(kh, kw) < 1 or max(kh, kw) > ops.VFE_MAX_KERNEL:
            raise NotImplementedError(f"the HIP VFE covers odd conv kernel sizes from 1 to {ops.VFE_MAX_KERNEL} in each "
                                      f"dimension, got {self.kernel_size}")
        if tuple(self.embedder[0].padding) != ((kh - 1) // 2, (kw - 1) // 2):
            raise NotImplementedError(f"the HIP VFE pads ((kh-1)/2, (kw-1)/2), the module has "
                                      f"{tuple(self.embedder[0].padding)}")
        if H > ops.VFE_MAX_H:
            raise NotImplementedError(f"the HIP VFE covers slice heights up to {ops.VFE_MAX_H}, got {H}")
        if (H * win_w) % 8:
            raise NotImplementedError(f"the HIP VFE bridge runs as a conv over slice_height * slice_width * stride = "
                                      f"{H * win_w} input channels, which must be a multiple of 8")
        if self._icassp() and self.slice_width <= 128:
            return
        lds = ops.vfe_stencil_lds_bytes(H, win_w, kh, kw)
        if lds > ops.VFE_LDS_MAX:
            raise NotImplementedError(f"the HIP VFE keeps a whole {H} x {win_w} context window (slice_width * stride "
                                      f"columns) in LDS: {lds} B with a {kh} x {kw} kernel, over the "
                                      f"{ops.VFE_LDS_MAX} B bound")

    def _build(self, device, dtype):
        convs, bns = [], []
        for m in self.embedder:
            if isinstance(m, nn.Conv2d):
                convs.append(torch.cat([m.weight.detach().float().reshape(-1), m.bias.detach().float()]))
                if not self.embed_normalize:
                    bns.append(torch.tensor([1.0, 0.0], device=m.weight.device))
            elif isinstance(m, nn.BatchNorm2d):
                s, sh = fold_bn(m)
                bns.append(torch.cat([s, sh]))
        lin = self._linear
        d = dict(conv=torch.stack(convs).to(device).contiguous(),
                 bn=torch.stack(bns).to(device).contiguous(),
                 w=ops.pack_conv_weight(lin.weight.to(device)[:, :, None], dtype),
                 b=lin.bias.detach().float().to(device).contiguous())
        # the bridge is a 2448-deep reduction over only B * n rows: as one conv each workgroup
        # walks 77 channel chunks in series (90 us at B = 32).  Split-K instead: S channel groups
        # as a grouped conv (group g = input channels [g Ci/S, (g+1) Ci/S) -> its own E outputs),
        # then the S partial sums are added in order (deterministic) -> 5 chunks per workgroup.
        E, Ci = lin.weight.shape
        S = next((s for s in (17, 16, 12, 8, 4, 2) if Ci % s == 0 and (Ci // s) % 8 == 0), 1)
        if S > 1:
            wg = lin.weight.detach().float().to(device).view(E, S, Ci // S).transpose(0, 1).reshape(S * E, Ci // S)
            d.update(split=S, wsplit=ops.pack_grouped_weight(wg[:, :, None], dtype, groups=S))
        return d

    def run(self, images, out_dtype=None):
        self._supported()
        p = self._packed(images.device, self._build)
        if self._icassp() and self.slice_width <= 128:
            flat, n = ops.vfe_stencil(images, p["conv"], p["bn"], self.slice_width, self.compute_dtype)
        else:
            flat, n = ops.vfe_stencil_ex(images, p["conv"], p["bn"], self.slice_width, self.stride, self.kernel_size,
                                         self.compute_dtype)
        B = images.shape[0]
        E = self.embed_dim
        if p.get("split", 1) > 1 and flat.shape[0] <= 4096:
            S = p["split"]
            part = ops.conv1d(flat.unsqueeze(0), p["wsplit"], None, Co=S * E, K=1, groups=S,
                              out_dtype=torch.float32, compute_dtype=self.compute_dtype)
            y = part.view(-1, S, E).sum(1) + p["b"]
            if self.bridge_relu:
                y = torch.relu(y)
            return y.to(out_dtype or self.compute_dtype).view(B, n, E)
        y = ops.conv1d(flat.unsqueeze(0), p["w"], p["b"], Co=E, K=1,
                       post_act=ops.ACT_RELU if self.bridge_relu else ops.ACT_NONE,
                       out_dtype=out_dtype or self.compute_dtype, compute_dtype=self.compute_dtype)
        return y.view(B, n, E)

    def train_run(self, images, out_dtype):
        """Training forward (BatchNorm2d uses batch statistics, so the eval-folded stencil kernel
        does not apply): the overlapping context windows gathered into (B n, 1, H, slice_w * stride)
        maps, then per layer conv (vo_vfe_conv / vo_vfe_conv_ex), BatchNorm with batch statistics
        (vo_bn_train_fwd) where configured, ReLU, and the bridge on HIP."""
        from .. import autograd as AG
        self._supported()
        B, C, H, W = images.shape
        win_w = self.slice_width * self.stride
        n = int((W - (self.stride // 2) * self.slice_width * 2) / self.slice_width)
        # window i = columns [i slice_w, i slice_w + win_w): (B, C, H, n, win_w) -> (B n, C, H, win_w)
        win = images.unfold(3, win_w, self.slice_width)[:, :, :, :n]
        x = win.permute(0, 3, 1, 2, 4).reshape(B * n, C, H, win_w)
        for m in self.embedder:
            if isinstance(m, nn.BatchNorm2d):
                x = AG.batch_norm_train(x, m, (0, 2, 3))
            elif isinstance(m, nn.ReLU):
                x = torch.relu(x)
            else:
                x = AG.vfe_conv(x, m)
        lin = self._linear
        y = AG.linear(x.reshape(1, B * n, -1).to(out_dtype), lin.weight, lin.bias,
                      relu=self.bridge_relu, compute_dtype=out_dtype)
        return y.view(B, n, self.embed_dim)

    def forward(self, images):
        self._check_inference()
        return self.run(images)
