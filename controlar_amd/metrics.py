"""Control consistency on the GPU: does a generated image obey the control it was given?  This is the scoring step of the reference's
``evaluations/canny_f1score.py``, ``hed_ssim.py``, ``lineart_ssim.py`` and ``depth_rmse.py`` and the accumulators of ``autoregressive/test/metric.py``,
without saved PNGs, torchmetrics, skimage or sklearn: ``car_ms_ssim``, ``car_f1``, ``car_rmse`` and ``car_pixels_to_u8`` behind ``Engine``.

``SSIM``, ``F1score`` and ``RMSE`` keep ``metric.py``'s call shape (``update(img1, img2)`` / ``calculate()``); ``ControlConsistency`` runs a whole
evaluation script for one batch: quantise as ``save_image`` does, re-extract the condition, score it against the control that was fed in."""
from __future__ import annotations

import numpy as np
import torch

from .config import tiny_t2i
from .engine import Engine

CONDITION_TYPES = ("canny", "hed", "lineart", "depth")


def _engine(engine, device=None) -> Engine:
    return engine if engine is not None else Engine(tiny_t2i(), "bf16", device=device)      # the kernels need no weights: any context serves


def _t(x) -> torch.Tensor:
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def _batched(x: torch.Tensor, lead: int) -> torch.Tensor:
    """[H,W] -> [1, (1,) H, W]; batches pass."""
    while x.dim() < lead:
        x = x[None]
    return x


class _Accumulator:
    """``update`` adds the batch mean and counts one, as the evaluation scripts append one value per batch; ``per_image`` keeps every value."""

    def __init__(self, engine=None, device=None):
        self._eng = _engine(engine, device)
        self.total = torch.zeros((), dtype=torch.float64, device=self._eng.device)
        self.count = 0
        self._values = []

    def _add(self, values: torch.Tensor) -> torch.Tensor:
        self._values.append(values)
        self.total = self.total + values.mean()
        self.count += 1
        return values

    @property
    def per_image(self) -> torch.Tensor:
        """Every image's value so far, fp64, in the order of the updates."""
        return torch.cat(self._values) if self._values else torch.empty(0, dtype=torch.float64, device=self._eng.device)

    def calculate(self) -> float:
        if self.count == 0:
            raise ValueError("No images have been added.")
        return float(self.total / self.count)


class SSIM(_Accumulator):
    """``metric.py``'s ``SSIM`` in call shape: raw 0..255 maps in, ``(img/255).clip(0,1)`` scored.  DEVIATION from ``metric.py``: that class builds the
    torchmetrics MS-SSIM object, drops it, and then calls skimage's single-scale ``structural_similarity``.  This one computes multi-scale SSIM, which is
    what every ``evaluations/*_ssim.py`` script and the paper report.  img1, img2: [H,W], [B,H,W] or [B,C,H,W], uint8 or float, sides >= 176."""

    def __init__(self, data_range=1.0, engine=None, device=None):
        super().__init__(engine, device)

    def update(self, img1, img2) -> torch.Tensor:
        a, b = _batched(_t(img1), 3), _batched(_t(img2), 3)
        return self._add(self._eng.ms_ssim(a, b, scale=1.0 / 255.0))


class F1score(_Accumulator):
    """``metric.py``'s ``F1score``: both maps are binarised with ``> threshold`` (128), F1 of the positive class (sklearn's ``f1_score``; 0 where
    neither map has a positive).  img1, img2: [H,W] or [B,H,W], uint8 or float."""

    def __init__(self, threshold=128, engine=None, device=None):
        super().__init__(engine, device)
        self.threshold = threshold

    def update(self, img1, img2) -> torch.Tensor:
        a, b = _batched(_t(img1), 3), _batched(_t(img2), 3)
        return self._add(self._eng.f1(b, a, threshold=self.threshold))           # metric.py: y_true from img1, y_pred from img2


class RMSE(_Accumulator):
    """``metric.py``'s ``RMSE``: sqrt(mean((img1 - img2)^2)) of the values as they are.  img1 float, img2 uint8 or float: [H,W] or [B,H,W]."""

    def update(self, img1, img2) -> torch.Tensor:
        a, b = _batched(_t(img1), 3), _batched(_t(img2), 3)
        return self._add(self._eng.rmse(a, b))


class ControlConsistency:
    """One evaluation script per condition type, on the device.  ``__call__(pixels, control)``: ``pixels`` [B,3,H,W] in [-1,1] straight from
    ``vq_decode``, ``control`` [B,3,H,W] in [-1,1] as it was fed to ``generate``.  Both are quantised as ``save_image(normalize=True,
    value_range=(-1,1))`` writes them (the scripts read those PNGs back); channel 0 of the control is the label.  Then, as the script for the type does:

    - ``'canny'``   ``CannyDetector`` at thresholds 100 / 200; F1 of the ``== 255`` maps                       (evaluations/canny_f1score.py)
    - ``'hed'``     ``HEDdetector`` output / 255 and label / 255, clipped; MS-SSIM                              (evaluations/hed_ssim.py)
    - ``'lineart'`` ``LineArt`` output as it is (0..1) and label / 255, clipped; MS-SSIM                        (evaluations/lineart_ssim.py)
    - ``'depth'``   ``DepthEstimator.preprocess(size=depth_size)``, the model, ``d * 255 / max``; RMSE against the label, which must have that size
                    (evaluations/depth_rmse.py; 512 x 512 there)

    ``extractor``: the ``condition.CannyDetector`` / ``HEDdetector`` / ``LineArt`` / ``DepthEstimator`` the caller already holds (its weights loaded);
    for ``'canny'`` a new one by default.  Returns ``(per_image fp64 [B], mean)``, both on the device; nothing is copied to the host."""

    def __init__(self, condition_type: str, extractor=None, depth_size=(512, 512), device=None):
        if condition_type not in CONDITION_TYPES:
            raise ValueError(f"condition_type {condition_type!r}: one of {CONDITION_TYPES}")
        if extractor is None:
            if condition_type != "canny":
                raise ValueError(f"condition_type {condition_type!r} needs the extractor that holds its weights (only 'canny' has none)")
            from .condition import CannyDetector
            extractor = CannyDetector(device=device)
        self.condition_type = condition_type
        self.extractor = extractor
        self.depth_size = (int(depth_size[0]), int(depth_size[1]))
        self._eng = extractor._eng             # the metric kernels need no weights: the extractor's context serves

    def extract(self, pixels: torch.Tensor) -> torch.Tensor:
        """The condition of ``pixels`` [B,3,H,W] in [-1,1], in the units the script scores: uint8 [B,H,W] edges (canny), fp32 [B,H,W] in 0..255 (hed),
        fp32 [B,1,Ho,Wo] in 0..1 (lineart), fp32 [B,S,S] predicted depth (depth)."""
        e, kind = self._eng, self.condition_type
        if kind == "canny":
            return e.canny(e.pixels_to_u8(pixels), 100, 200)
        if kind == "hed":
            return e.hed(e.pixels_to_u8(pixels, want_float=True)[1])
        if kind == "lineart":
            return e.lineart(e.pixels_to_u8(pixels, want_float=True)[1])
        pv = self.extractor.preprocess(e.pixels_to_u8(pixels).permute(0, 3, 1, 2), size=self.depth_size)
        return e.depth(pv)

    def label(self, control: torch.Tensor) -> torch.Tensor:
        """Channel 0 of the control image as ``save_image`` writes it: uint8 [B,H,W]."""
        return self._eng.pixels_to_u8(control)[..., 0].contiguous()

    def __call__(self, pixels: torch.Tensor, control: torch.Tensor):
        e, kind = self._eng, self.condition_type
        got, want = self.extract(pixels), self.label(control)
        if tuple(got.shape[-2:]) != tuple(want.shape[-2:]):
            raise ValueError(f"the re-extracted {kind} map is {tuple(got.shape[-2:])} and the control is {tuple(want.shape[-2:])}: the script compares them pixel by pixel")
        if kind == "canny":
            vals = e.f1(got, want, value=255)
        elif kind == "hed":
            vals = e.ms_ssim(got[:, None], want[:, None], scale=(1.0 / 255.0, 1.0 / 255.0))
        elif kind == "lineart":
            vals = e.ms_ssim(got, want[:, None], scale=(1.0, 1.0 / 255.0))
        else:
            vals = e.rmse(got, want, scale_to_max=True)
        return vals, vals.mean()


class CLIPScore:
    """Prompt alignment as ``compute_clip_score`` reports it (evaluations/t2i/evaluation.py:129-176): the cosine between CLIP's image and text
    embeddings of every pair, and the mean over the first ``how_many`` pairs in the order they came, which is where the script cuts.  ``scorer``: a
    ``clip.CLIPScorer`` (its weights loaded).  ``update(pixels, ids)``: ``pixels`` [B,3,H,W] in [-1,1] straight from ``vq_decode``, ``ids`` [B,T] as
    ``clip.photo_depicts_ids`` leaves them; returns the batch's fp32 cosines.  Everything stays on the device until ``calculate()``."""

    def __init__(self, scorer, how_many: int = 5000, eval_res: int = 256):
        if how_many < 1:
            raise ValueError(f"how_many must be at least 1, got {how_many}")
        self.scorer = scorer
        self.how_many = int(how_many)
        self.eval_res = int(eval_res)
        self._values = []

    def update(self, pixels: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
        vals = self.scorer.score(pixels, ids, eval_res=self.eval_res)
        self._values.append(vals)
        return vals

    @property
    def per_image(self) -> torch.Tensor:
        """Every pair's cosine so far, fp32, in the order of the updates."""
        return torch.cat(self._values) if self._values else torch.empty(0, dtype=torch.float32, device=self.scorer.device)

    def calculate(self) -> float:
        vals = self.per_image
        if vals.numel() == 0:
            raise ValueError("No images have been added.")
        return float(vals[:self.how_many].to(torch.float64).mean())          # one scalar leaves the device: the script's torch.cat(...)[:how_many].mean()


class PSNR(_Accumulator):
    """PSNR in ``metric.py``'s call shape: ``update(img1, img2)`` adds skimage's ``peak_signal_noise_ratio`` of every image, as the tokenizer evaluation
    collects it (tokenizer/tokenizer_image/reconstruction_vq_ddp.py:149-153).  img1, img2: [B,...] of one shape, uint8 (read as v / 255) or float in
    0..data_range.  Equal images give +inf, as skimage does."""

    def __init__(self, data_range=1.0, engine=None, device=None):
        super().__init__(engine, device)
        self.data_range = float(data_range)

    def update(self, img1, img2) -> torch.Tensor:
        return self._add(self._eng.psnr(_t(img1), _t(img2), data_range=self.data_range))


class LPIPS(_Accumulator):
    """The reference's ``LPIPS().eval()`` (tokenizer/tokenizer_image/lpips.py:53-96) as an accumulator: ``update(img1, img2)`` on [B,3,H,W] in [-1,1].
    ``engine`` holds the weights (``Engine.load_lpips``), or ``weights`` (a local checkpoint path or a state dict, see ``read_lpips_weights``) are loaded into
    it; nothing is ever downloaded."""

    def __init__(self, weights=None, engine=None, device=None):
        super().__init__(engine, device)
        if weights is not None:
            self._eng.load_lpips(read_lpips_weights(weights))

    def update(self, img1, img2) -> torch.Tensor:
        return self._add(self._eng.lpips(_t(img1), _t(img2)))


def read_lpips_weights(weights):
    """A state dict for ``Engine.load_lpips`` from a state dict, a local file ``torch.load`` reads, or a list / tuple of those merged in order — the
    real network comes in two files, torchvision's VGG-16 (``features.N.*``; its ``classifier.*`` tensors are dropped) and the LPIPS ``vgg.pth`` with
    the ``lin`` layers.  The reference's constructor fetches both (lpips.py:59,69-72); this never does."""
    if isinstance(weights, (list, tuple)):
        merged = {}
        for w in weights:
            merged.update(read_lpips_weights(w))
        return merged
    sd = torch.load(weights, map_location="cpu") if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__") else dict(weights)
    return {k: v for k, v in sd.items() if not k.startswith("classifier.")}


class ReconstructionQuality:
    """The tokenizer evaluation of tokenizer/tokenizer_image/reconstruction_vq_ddp.py:128-155 for one batch, on the device, plus the LPIPS the tokenizer
    is trained against (vq_loss.py:93-95).  ``engine`` holds the VQ weights (``__call__``) in the arithmetic to be judged; ``lpips_weights``: a local
    path, a state dict or a list of them (``read_lpips_weights``), loaded into ``lpips_engine`` (default: ``engine`` itself; pass an fp32 context to judge a
    bf16 decoder with an exact LPIPS).  ``__call__(images)``, images [B,3,H,W] in [-1,1]: ``vq_encode``, ``vq_decode``, the script's quantiser, PSNR of
    quantised / 255 against (x + 1) / 2, LPIPS between x and the decoded pixels.  ``compare(pixels_a, pixels_b)`` scores one decoder's pixels against
    another's the same way.  Both return a dict of fp64 [B] tensors ``psnr`` and ``lpips`` plus the intermediate tensors; nothing leaves the device."""

    def __init__(self, engine: Engine, lpips_weights=None, lpips_engine: Engine = None):
        self._eng = engine
        self._lp = lpips_engine if lpips_engine is not None else engine
        if lpips_weights is not None:
            self._lp.load_lpips(read_lpips_weights(lpips_weights))

    def _score(self, x: torch.Tensor, pixels: torch.Tensor) -> dict:
        e = self._eng
        u8 = e.recon_to_u8(pixels)
        return {"psnr": e.psnr(u8, x, data_range=1.0, a_map="div255", b_map="half"), "lpips": self._lp.lpips(x, pixels), "pixels": pixels, "u8": u8}

    def __call__(self, images: torch.Tensor) -> dict:
        e = self._eng
        x = images.to(device=e.device, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        down = 2 ** (len(e.cfg.vq.ch_mult) - 1)
        tokens = e.vq_encode(x)
        res = self._score(x, e.vq_decode(tokens, H // down, W // down))
        res["tokens"] = tokens
        return res

    def compare(self, pixels_a: torch.Tensor, pixels_b: torch.Tensor) -> dict:
        """``pixels_b`` judged against ``pixels_a`` (both [B,3,H,W] in [-1,1], e.g. the fp32 and the bf16 decoder on the same tokens): PSNR of quantised
        b / 255 against (a + 1) / 2, LPIPS(a, b).  ``compare(p, p)`` gives LPIPS exactly 0."""
        e = self._eng
        a = pixels_a.to(device=e.device, dtype=torch.float32).contiguous()
        return self._score(a, pixels_b.to(device=e.device, dtype=torch.float32).contiguous())


# ---------------------------------------------------------------------- sample quality: evaluations/c2i/evaluator.py from compute_statistics down
def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """``FIDStatistics(mu1, sigma1).frechet_distance(FIDStatistics(mu2, sigma2), eps)`` (evaluations/c2i/evaluator.py:84-127) on the host, with the same
    numpy / scipy calls in the same order: ``linalg.sqrtm`` of the product, the retry with ``eps`` on both diagonals where that is not finite, the
    check of the imaginary part, ``diff.dot(diff) + trace + trace - 2 trace``.  One D^3 matrix square root per evaluation: not a device path."""
    import warnings
    try:
        from scipy import linalg
    except ImportError as e:
        raise ImportError("frechet_distance needs scipy (scipy.linalg.sqrtm), which is not installed") from e
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    if mu1.shape != mu2.shape:
        raise ValueError(f"the mean vectors differ in length: {mu1.shape}, {mu2.shape}")
    if sigma1.shape != sigma2.shape:
        raise ValueError(f"the covariances differ in shape: {sigma1.shape}, {sigma2.shape}")
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        warnings.warn("fid calculation produces singular product; adding %s to diagonal of cov estimates" % eps)
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


class FeatureStatistics:
    """``Evaluator.compute_statistics`` (evaluator.py:186-189) as a running state on the device: ``update(acts)`` adds a batch [n, D] in fp64 on the matrix
    cores, ``finalize()`` returns ``(mu, sigma)`` = ``np.mean(axis=0)``, ``np.cov(rowvar=False)`` as fp64 device tensors.  The same updates give the same
    bits.  (The script's ``mu`` is an fp32 ``np.mean`` of fp32 activations; this one is fp64.)"""

    def __init__(self, engine=None, device=None):
        self._eng = _engine(engine, device)
        self._state = None
        self._D = None

    def update(self, acts) -> None:
        x = _t(acts)
        if self._state is None:
            self._D = int(x.shape[1])
            self._state = self._eng.fid_state(self._D)
        elif x.dim() != 2 or x.shape[1] != self._D:
            raise ValueError(f"update: expected [n, {self._D}], got {tuple(x.shape)}")
        self._eng.fid_accumulate(self._state, x)

    def finalize(self):
        if self._state is None:
            raise ValueError("No activations have been added.")
        return self._eng.fid_finalize(self._state, self._D)


class InceptionScore:
    """``Evaluator.compute_inception_score`` (evaluator.py:191-204): ``InceptionScore(w)(acts)`` with the softmax weight ``w`` [D, C] of the Inception graph
    (``_create_softmax_graph``: the last layer without its bias).  ``last_splits`` keeps the per-split values (a device tensor)."""

    def __init__(self, w, split_size=5000, engine=None, device=None):
        self._eng = _engine(engine, device)
        self._w = _t(w).to(device=self._eng.device, dtype=torch.float32).contiguous()
        self.split_size = int(split_size)
        self.last_splits = None

    def __call__(self, acts) -> float:
        out = self._eng.inception_score(_t(acts), self._w, self.split_size)
        self.last_splits = out[1:]
        return float(out[0])


class PrecisionRecall:
    """``Evaluator.compute_prec_recall`` (evaluator.py:206-214) with the ``ManifoldEstimator`` defaults: ``PrecisionRecall()(ref_acts, sample_acts)`` ->
    ``(precision, recall)``.  ``radii`` and ``status`` of the last call stay available as device tensors."""

    def __init__(self, k=3, row_batch=10000, col_batch=10000, engine=None, device=None):
        self._eng = _engine(engine, device)
        self.k, self.row_batch, self.col_batch = int(k), int(row_batch), int(col_batch)
        self.radii = self.status = None

    def __call__(self, ref_acts, sample_acts):
        e = self._eng
        a, b = _t(ref_acts).to(e.device), _t(sample_acts).to(e.device)
        r1 = e.manifold_radii(a, self.k, self.row_batch, self.col_batch)
        r2 = e.manifold_radii(b, self.k, self.row_batch, self.col_batch)
        s1, s2, pr = e.manifold_pr(a, r1, b, r2, self.row_batch, self.col_batch)
        self.radii, self.status = (r1, r2), (s1, s2)
        p = pr.cpu()
        return float(p[0]), float(p[1])


class SampleQuality:
    """The five numbers of evaluations/c2i/evaluator.py's ``main`` from activations that are already on the device (the Inception tower that produces them
    is not part of this package).  The reference side is either activations (``ref_acts`` [N, D], and ``ref_acts_spatial`` for sFID) or the precomputed
    moments the published reference batches carry (``ref_stats=(mu, sigma)``, ``ref_stats_spatial=(mu_s, sigma_s)``); precision and recall need
    ``ref_acts``.  ``__call__(sample_acts, sample_acts_spatial=None, softmax_weight=None)`` returns a dict with ``inception_score``, ``fid``, ``sfid``,
    ``precision`` and ``recall`` (``None`` for what its inputs were not given).  Activations never leave the device; the two moment pairs go to the
    host for ``frechet_distance``."""

    def __init__(self, ref_acts=None, ref_stats=None, ref_acts_spatial=None, ref_stats_spatial=None, softmax_weight=None, split_size=5000, k=3,
                 row_batch=10000, col_batch=10000, batch=10000, engine=None, device=None):
        self._eng = _engine(engine, device)
        self._batch = int(batch)
        self._ref_acts = None if ref_acts is None else _t(ref_acts).to(self._eng.device)
        self._w, self._split = softmax_weight, split_size
        self._pr = PrecisionRecall(k, row_batch, col_batch, engine=self._eng)
        self._ref = self._host(ref_stats) if ref_stats is not None else (self._moments(self._ref_acts) if self._ref_acts is not None else None)
        self._ref_s = (self._host(ref_stats_spatial) if ref_stats_spatial is not None
                       else (self._moments(_t(ref_acts_spatial)) if ref_acts_spatial is not None else None))

    @staticmethod
    def _host(stats):
        mu, sigma = stats
        return tuple(np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v) for v in (mu, sigma))

    def _moments(self, acts):
        fs = FeatureStatistics(engine=self._eng)
        for i in range(0, acts.shape[0], self._batch):
            fs.update(acts[i:i + self._batch])
        return self._host(fs.finalize())

    def __call__(self, sample_acts, sample_acts_spatial=None, softmax_weight=None) -> dict:
        x = _t(sample_acts).to(self._eng.device)
        w = softmax_weight if softmax_weight is not None else self._w
        res = {"inception_score": None, "fid": None, "sfid": None, "precision": None, "recall": None}
        if w is not None:
            res["inception_score"] = InceptionScore(w, self._split, engine=self._eng)(x)
        if self._ref is not None:
            res["fid"] = float(frechet_distance(*self._moments(x), *self._ref))
        if self._ref_s is not None and sample_acts_spatial is not None:
            res["sfid"] = float(frechet_distance(*self._moments(_t(sample_acts_spatial)), *self._ref_s))
        if self._ref_acts is not None:
            res["precision"], res["recall"] = self._pr(self._ref_acts, x)
        return res
