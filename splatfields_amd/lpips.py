"""LPIPS (VGG) on the device: the third number of the reference's ``eval_all`` (render.py:163-207), for a batch of views.

The arithmetic is the published ``lpips`` package, v0.1, ``net='vgg'``, ``spatial=False``, eval mode: a scaling layer, the 13
convolutions of the VGG-16 trunk with a max-pool between its five groups, and at the last ReLU of every group a distance of the
channel-normalised features, weighted per channel and averaged over the pixels (csrc/lpips.hip states the formula).  It is
restated from the package's published behaviour: neither the package nor its weights are available to this repository, so
nothing here has been compared with them, and the repository holds no weights of any published network -- ``LPIPSWeights``
is built from tensors the caller supplies (``from_state_dict`` for the published layout) or from a random recipe
(``LPIPSWeights.random``) that the tests and the benchmark use.

``lpips_vgg`` takes what ``image_metrics`` takes (both layouts by strides, the 8-bit quantisation in the kernel), runs pred and
gt of every item through the same 13 convolution launches (float32 on ``v_mfma_f32_32x32x2_f32``), 5 head launches and one
fixed-order reduction per chunk of the batch, never waits for the device and returns bit-identical results from call to call
and whatever the chunking.  There is no CPU path and nothing is differentiable."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import ptr
from .metrics import _QUANT, _check_pair, _f32, _strides4

CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
MIN_SIDE = 16                      # relu5_3 has no pixel below
LAUNCHES_PER_CHUNK = 19            # csrc/lpips.hip: 13 convolutions + 5 heads + 1 reduction
DEFAULT_WORKSPACE_CAP = 4 << 30    # bytes: five pairs of 800 x 800 per chunk
# the published state dict, as recalled: the indices of the trunk's convolutions inside torchvision's vgg16().features
TRUNK_KEYS = ("net.slice1.0", "net.slice1.2", "net.slice2.5", "net.slice2.7", "net.slice3.10", "net.slice3.12", "net.slice3.14",
              "net.slice4.17", "net.slice4.19", "net.slice4.21", "net.slice5.24", "net.slice5.26", "net.slice5.28")
LIN_KEYS = tuple(f"lin{i}.model.1.weight" for i in range(5))
SHIFT_KEY, SCALE_KEY = "scaling_layer.shift", "scaling_layer.scale"


class LPIPSWeights:
    """The weights of the network: 13 (weight [cout,cin,3,3], bias [cout]) pairs, 5 ``lin`` vectors ([C] or [1,C,1,1]) and the
    scaling layer's shift and scale ([3], or anything with 3 elements; default: the published constants).  Every shape is
    checked here.  The tensors may live on any device; the kernels' layout is packed once, on the first evaluation, on the
    device the tensors are on."""

    def __init__(self, convs: Sequence, lins: Sequence, shift=None, scale=None):
        convs, lins = list(convs), list(lins)
        if len(convs) != len(CONV_CHANNELS):
            raise ValueError(f"LPIPSWeights: {len(CONV_CHANNELS)} (weight, bias) pairs are required, got {len(convs)}")
        if len(lins) != len(TAP_CHANNELS):
            raise ValueError(f"LPIPSWeights: {len(TAP_CHANNELS)} lin vectors are required, got {len(lins)}")
        dev = convs[0][0].device
        self.convs = []
        for i, ((w, b), (cin, cout)) in enumerate(zip(convs, CONV_CHANNELS)):
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise ValueError(f"LPIPSWeights: convolution {i} must be [{cout},{cin},3,3] with a bias [{cout}], got {tuple(w.shape)} "
                                 f"and {tuple(b.shape)}")
            self.convs.append((_lib.f32c(w), _lib.f32c(b)))
        self.lins = []
        for i, (v, c) in enumerate(zip(lins, TAP_CHANNELS)):
            if tuple(v.shape) not in ((c,), (1, c, 1, 1)):
                raise ValueError(f"LPIPSWeights: lin {i} must have {c} weights ([{c}] or [1,{c},1,1]), got {tuple(v.shape)}")
            self.lins.append(_lib.f32c(v).reshape(c))
        consts = []
        for name, v, default in (("shift", shift, SHIFT), ("scale", scale, SCALE)):
            v = torch.tensor(default, dtype=torch.float32, device=dev) if v is None else _lib.f32c(torch.as_tensor(v))
            if v.numel() != 3:
                raise ValueError(f"LPIPSWeights: {name} must have 3 elements, got {tuple(v.shape)}")
            consts.append(v.reshape(3).contiguous())
        self.shift, self.scale = consts
        tensors = [t for pair in self.convs for t in pair] + self.lins + consts
        if any(t.device != dev for t in tensors):
            raise ValueError("LPIPSWeights: all tensors must be on one device")
        self.device = dev
        self._packed = None

    def to(self, device) -> "LPIPSWeights":
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self
        return LPIPSWeights([(w.to(device), b.to(device)) for w, b in self.convs], [v.to(device) for v in self.lins],
                            self.shift.to(device), self.scale.to(device))

    @classmethod
    def random(cls, seed: int, device=None) -> "LPIPSWeights":
        """He-scaled random weights for tests and the benchmark: w ~ N(0, 2 / (9 cin)), b ~ 0.05 N(0, 1), lin ~ U(0, 4 / C), the
        published shift and scale.  Drawn on the CPU, so the same seed gives the same weights on every device."""
        g = torch.Generator().manual_seed(int(seed))
        convs = [(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5, 0.05 * torch.randn(cout, generator=g))
                 for cin, cout in CONV_CHANNELS]
        lins = [torch.rand(c, generator=g) * (4.0 / c) for c in TAP_CHANNELS]
        w = cls(convs, lins)
        return w if device is None else w.to(device)

    @classmethod
    def from_state_dict(cls, sd) -> "LPIPSWeights":
        """From the state dict of the published ``lpips.LPIPS(net='vgg')``, whose keys are, AS RECALLED: the trunk
        ``net.slice1.{0,2}``, ``net.slice2.{5,7}``, ``net.slice3.{10,12,14}``, ``net.slice4.{17,19,21}``,
        ``net.slice5.{24,26,28}``, each with ``.weight`` / ``.bias``; ``lin{0..4}.model.1.weight`` of shape [1,C,1,1];
        ``scaling_layer.shift`` / ``scaling_layer.scale``.  These names are unverified here: the package is not available to this
        repository.  Raises KeyError naming every key it could not find, ValueError for a wrong shape."""
        need = [k + s for k in TRUNK_KEYS for s in (".weight", ".bias")] + list(LIN_KEYS) + [SHIFT_KEY, SCALE_KEY]
        missing = [k for k in need if k not in sd]
        if missing:
            raise KeyError(f"LPIPSWeights.from_state_dict: keys not found: {', '.join(missing)}")
        return cls([(sd[k + ".weight"], sd[k + ".bias"]) for k in TRUNK_KEYS], [sd[k] for k in LIN_KEYS], sd[SHIFT_KEY], sd[SCALE_KEY])

    def state_dict(self) -> dict:
        """the layout `from_state_dict` reads"""
        sd = {}
        for k, (w, b) in zip(TRUNK_KEYS, self.convs):
            sd[k + ".weight"], sd[k + ".bias"] = w, b
        for k, v in zip(LIN_KEYS, self.lins):
            sd[k] = v.reshape(1, -1, 1, 1)
        sd[SHIFT_KEY], sd[SCALE_KEY] = self.shift.reshape(1, 3, 1, 1), self.scale.reshape(1, 3, 1, 1)
        return sd

    def packed(self) -> torch.Tensor:
        """the device blob in the kernels' layout (sr_lpips_pack_weights), made once"""
        if self._packed is None:
            if self.device.type != "cuda":
                raise RuntimeError("LPIPSWeights has no CPU path: move the weights to a HIP ('cuda') device with .to()")
            lib = _lib.load()
            table = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            with torch.cuda.device(self.device):
                blob = torch.empty(lib.sr_lpips_packed_bytes(), dtype=torch.uint8, device=self.device)
                _lib.check(lib.sr_lpips_pack_weights(table([w for w, _ in self.convs]), table([b for _, b in self.convs]), table(self.lins),
                                                     ptr(self.shift), ptr(self.scale), ptr(blob), _lib.stream(self.device)))
            self._packed = blob
        return self._packed


def _as_weights(loss_fn_vgg) -> LPIPSWeights:
    """an LPIPSWeights, or a module with a state_dict() in the published layout: converted once, cached on the object"""
    if isinstance(loss_fn_vgg, LPIPSWeights):
        return loss_fn_vgg
    cached = getattr(loss_fn_vgg, "_splatfields_lpips_weights", None)
    if cached is None:
        if not hasattr(loss_fn_vgg, "state_dict"):
            raise TypeError("lpips: expected an LPIPSWeights or a module with a state_dict()")
        cached = LPIPSWeights.from_state_dict(loss_fn_vgg.state_dict())
        loss_fn_vgg._splatfields_lpips_weights = cached
    return cached


def lpips_vgg(pred: torch.Tensor, gt: torch.Tensor, weights: LPIPSWeights, *, layout: str = "chw", quantize: Optional[str] = None,
              return_taps: bool = False, return_maps: bool = False, max_workspace_bytes: int = DEFAULT_WORKSPACE_CAP):
    """LPIPS (VGG) of one image pair or a batch, on the device.

    pred, gt   [3,H,W] / [B,3,H,W] with ``layout="chw"``, [H,W,3] / [B,H,W,3] with ``"hwc"``; values in [0,1], any strides,
               H and W at least 16.
    quantize   None, ``"png"`` or ``"to8b"``: both images go through the 8-bit round trip first, as in ``image_metrics``.
    max_workspace_bytes  the batch is processed in chunks whose workspace fits; the chunking changes no bit of any item.
    -> [B] float32 (0-dim for one image); with ``return_taps`` ``(values, taps [B,5])``; with ``return_maps`` (for tests)
    ``(values, taps, [five per-pixel maps [B, H >> l, W >> l]])``."""
    _check_pair("lpips_vgg", pred, gt)
    if not isinstance(weights, LPIPSWeights):
        raise TypeError("lpips_vgg: weights must be an LPIPSWeights")
    if layout not in ("chw", "hwc"):
        raise ValueError(f"lpips_vgg: layout must be 'chw' or 'hwc', got {layout!r}")
    if quantize not in _QUANT:
        raise ValueError(f"lpips_vgg: quantize must be None, 'png' or 'to8b', got {quantize!r}")
    if pred.dim() not in (3, 4):
        raise RuntimeError(f"lpips_vgg: expected one image or a batch of images, got {tuple(pred.shape)}")
    single = pred.dim() == 3
    x, y = _f32(pred), _f32(gt)
    if single:
        x, y = x[None], y[None]
    batch = x.shape[0]
    channels, h, w = (x.shape[1], x.shape[2], x.shape[3]) if layout == "chw" else (x.shape[3], x.shape[1], x.shape[2])
    if channels != 3:
        raise RuntimeError(f"lpips_vgg: RGB images are required, got {channels} channels in layout {layout!r} for {tuple(pred.shape)}")
    if batch == 0:
        raise RuntimeError("lpips_vgg: an empty batch")
    if h < MIN_SIDE or w < MIN_SIDE:
        raise ValueError(f"lpips_vgg: relu5_3 needs images of at least {MIN_SIDE} x {MIN_SIDE}, got {h} x {w}")
    dev = x.device
    if weights.device != dev:
        raise RuntimeError(f"lpips_vgg: the weights are on {weights.device}, the images on {dev}")
    lib = _lib.load()
    one = lib.sr_lpips_workspace_bytes(1, h, w)
    if one == 0:
        raise ValueError(f"lpips_vgg: images of {h} x {w} are too large")
    if one > max_workspace_bytes:
        raise ValueError(f"lpips_vgg: one pair of {h} x {w} needs a workspace of {one} bytes, max_workspace_bytes is {max_workspace_bytes}")
    chunk = min(batch, max(1, max_workspace_bytes // one))
    while chunk > 1 and not 0 < lib.sr_lpips_workspace_bytes(chunk, h, w) <= max_workspace_bytes:
        chunk -= 1
    want_taps = return_taps or return_maps
    packed = weights.packed()
    with torch.cuda.device(dev):
        work = torch.empty(lib.sr_lpips_workspace_bytes(chunk, h, w), dtype=torch.uint8, device=dev)
        out = torch.empty(batch, dtype=torch.float32, device=dev)
        taps = torch.empty((batch, len(TAP_CHANNELS)), dtype=torch.float32, device=dev) if want_taps else None
        maps = [torch.empty((batch, h >> l, w >> l), dtype=torch.float32, device=dev) for l in range(len(TAP_CHANNELS))] if return_maps else None
        for i0 in range(0, batch, chunk):
            i1 = min(batch, i0 + chunk)
            xs, ys = x[i0:i1], y[i0:i1]
            flat = torch.empty(lib.sr_lpips_maps_floats(i1 - i0, h, w), dtype=torch.float32, device=dev) if return_maps else None
            _lib.check(lib.sr_lpips_forward(i1 - i0, h, w, ptr(xs), _strides4(xs, layout), ptr(ys), _strides4(ys, layout), _QUANT[quantize],
                                            ptr(packed), ptr(work), ptr(out[i0:i1]), ptr(taps[i0:i1]) if want_taps else None, ptr(flat),
                                            _lib.stream(dev)))
            if return_maps:
                at = 0
                for l, m in enumerate(maps):
                    n = (i1 - i0) * (h >> l) * (w >> l)
                    m[i0:i1] = flat[at:at + n].reshape(i1 - i0, h >> l, w >> l)
                    at += n
    if single:
        out = out[0]
        taps = taps[0] if want_taps else None
        maps = [m[0] for m in maps] if return_maps else None
    if return_maps:
        return out, taps, maps
    return (out, taps) if return_taps else out


def eval_lpips(img0: torch.Tensor, img1: torch.Tensor, loss_fn_vgg) -> torch.Tensor:
    """The reference's ``eval_lpips`` (render.py:174-180): [H,W,3] images in [0,1] -> the value, a 0-dim tensor.  ``loss_fn_vgg``
    is an ``LPIPSWeights``, or any module with a ``state_dict()`` in the published layout (``LPIPSWeights.from_state_dict``),
    which is converted once and cached on the object."""
    _check_pair("eval_lpips", img0, img1)
    if img0.dim() != 3 or img0.shape[-1] != 3:
        raise RuntimeError(f"eval_lpips: expected [H,W,3] images, got {tuple(img0.shape)}")
    return lpips_vgg(img0, img1, _as_weights(loss_fn_vgg), layout="hwc").to(img0.dtype)
