"""Exact t-SNE of sampled pixel features: the reference's ``demo_tsne`` mode (utils/tsne_visualization.py), which hands up to
1000 features per class to ``tsne_torch`` (van der Maaten's tsne.py in eager torch, about ten N x N tensors per iteration).

``tsne_exact`` restates tsne.py (its constants; include/dcl_tsne.h spells the arithmetic out).  For CUDA fp32 input it runs on
libdcl_tsne.so (csrc/dcl_tsne.hip): P [N, N] is the only N x N buffer and an iteration reads it once.  Everything else (CPU
tensors, other dtypes, ``DCL_TSNE_HIP=0``, N * N >= 2^31) takes the torch composition below: the same arithmetic in the input's
dtype, evaluated in row chunks so that here too no N x N tensor other than P exists.  The composition in float64 is the tests'
reference.

Stated deviations from tsne.py / the reference's manager:
  * the PCA to 50 dimensions is skipped for D <= 50 (a rotation leaves the distances unchanged); for D > 50 it is an ``eigh`` of
    the covariance in float64 with each eigenvector's largest-magnitude component made positive;
  * a row's squared distances are shifted by their minimum before the search for beta (neutral in exact arithmetic; without it
    ``exp`` underflows to a zero sum on unnormalised inputs, which tsne.py turns into NaN);
  * ``Y0`` and the sampling permutations come from generators of their own, seeded from the config, not from the global one;
  * datasets other than Cityscapes sample ``feats_per_class // 500`` pixels per class and image (the reference raises there);
  * the scatter plot is drawn with PIL in the colours of ``utils.predict.class_palette``; an ``.npz`` with the numbers lies beside it.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from ..debug import cfg as _dbg

PCA_DIMS = 50
TOL = 1e-5
MAX_TRIES = 50
ETA = 500.0
MIN_GAIN = 0.01
CHUNK_ELEMS = 1 << 22            # elements of a [rows, N] temporary of the composition


def _row_chunks(n):
    rows = max(1, min(n, CHUNK_ELEMS // max(n, 1)))
    return [(r0, min(n, r0 + rows)) for r0 in range(0, n, rows)]


def exaggeration(it):
    return 4.0 if it <= 100 else 1.0


def momentum(it):
    return 0.5 if it < 20 else 0.8


# ---- step 1 ---------------------------------------------------------------------------------------------------------------------
def pca(X, dims=PCA_DIMS):
    """X [N, D] projected onto the ``dims`` leading eigenvectors of its covariance (float64 ``eigh``, signs fixed); X itself for
    D <= dims."""
    if X.shape[1] <= dims:
        return X
    Xc = X.detach().to(torch.float64)
    Xc = Xc - Xc.mean(0, keepdim=True)
    _, vec = torch.linalg.eigh((Xc.T @ Xc).cpu())           # ascending eigenvalues; D x D, on the host
    vec = vec.to(Xc.device)
    vec = vec[:, -dims:].flip(1)
    top = vec.abs().argmax(0)
    vec = vec * torch.sign(vec[top, torch.arange(dims, device=vec.device)])
    return (Xc @ vec).to(X.dtype).contiguous()


# ---- steps 2 and 3: the composition ---------------------------------------------------------------------------------------------
def shifted_sq_distances(X, r0, r1):
    """[r1 - r0, N]: d_j = sum_k (x_ik - x_jk)^2 of rows [r0, r1), minus the row's minimum over j != i; 0 on the diagonal."""
    c = r1 - r0
    d = X.new_zeros((c, X.shape[0]))
    for k in range(X.shape[1]):
        diff = X[r0:r1, k, None] - X[None, :, k]
        d.addcmul_(diff, diff)
    ar = torch.arange(c, device=X.device)
    d[ar, r0 + ar] = math.inf
    d -= d.min(1, keepdim=True).values
    d[ar, r0 + ar] = 0
    return d


def entropy_at(d, beta, r0):
    """(H [c], E [c, N], sum E [c]) of shifted distances d (rows r0 ...) at beta [c]; the diagonal carries no weight."""
    ar = torch.arange(d.shape[0], device=d.device)
    E = torch.exp(-beta[:, None] * d)
    E[ar, r0 + ar] = 0
    sp = E.sum(1)
    H = torch.log(sp) + beta * (d * E).sum(1) / sp
    return H, E, sp


def cond_p(X, perplexity):
    """(P [N, N], beta [N]) of step 2 in X's dtype: every row searched as tsne.py's x2p does, the rows of a chunk side by side."""
    N = X.shape[0]
    P = X.new_empty((N, N))
    beta_out = X.new_empty(N)
    log_u = math.log(perplexity)
    for r0, r1 in _row_chunks(N):
        d = shifted_sq_distances(X, r0, r1)
        c = r1 - r0
        beta = X.new_ones(c)
        lo, hi = X.new_full((c,), -math.inf), X.new_full((c,), math.inf)
        active = torch.ones(c, dtype=torch.bool, device=X.device)
        for tries in range(MAX_TRIES + 1):
            H, E, sp = entropy_at(d, beta, r0)
            diff = H - log_u
            active = active & (diff.abs() > TOL)            # a row that met the tolerance has left its loop
            if tries == MAX_TRIES or not bool(active.any()):
                break
            up, down = active & (diff > 0), active & ~(diff > 0)
            lo, hi = torch.where(up, beta, lo), torch.where(down, beta, hi)
            beta = torch.where(up, torch.where(torch.isinf(hi), beta * 2, (beta + hi) / 2),
                               torch.where(down, torch.where(torch.isinf(lo), beta / 2, (beta + lo) / 2), beta))
        P[r0:r1] = E / sp[:, None]
        beta_out[r0:r1] = beta
    return P, beta_out


def symmetrize_(P):
    """P <- (P + P^T) / sum(P + P^T), in place, tile pair by tile pair (no second N x N tensor)."""
    N = P.shape[0]
    chunks = _row_chunks(N)
    total = P.new_zeros(())
    for i, (r0, r1) in enumerate(chunks):
        for (c0, c1) in chunks[i:]:
            s = P[r0:r1, c0:c1] + P[c0:c1, r0:r1].T
            total = total + (s.sum() if r0 == c0 else 2 * s.sum())
            P[r0:r1, c0:c1] = s
            if r0 != c0:
                P[c0:c1, r0:r1] = s.T
    P /= total
    return P


# ---- step 5: the composition ----------------------------------------------------------------------------------------------------
def _num(Y, r0, r1):
    dx, dy = Y[r0:r1, 0, None] - Y[None, :, 0], Y[r0:r1, 1, None] - Y[None, :, 1]
    num = 1 / (1 + dx * dx + dy * dy)
    ar = torch.arange(r1 - r0, device=Y.device)
    num[ar, r0 + ar] = 0
    return num, dx, dy


def z_sum(Y):
    total = Y.new_zeros(())
    for r0, r1 in _row_chunks(Y.shape[0]):
        total = total + _num(Y, r0, r1)[0].sum()
    return total


def gradient(P, Y, exagg, want_kl=False):
    """(dY [N, 2], Z, KL or None) of one iteration at exaggeration ``exagg`` (4 or 1)."""
    Z = z_sum(Y)
    dY = torch.empty_like(Y)
    kl = Y.new_zeros(()) if want_kl else None
    for r0, r1 in _row_chunks(Y.shape[0]):
        num, dx, dy = _num(Y, r0, r1)
        p = (4 * P[r0:r1]).clamp_(min=1e-21) * (exagg / 4)
        q = (num / Z).clamp_(min=1e-12)
        w = (p - q) * num
        dY[r0:r1, 0], dY[r0:r1, 1] = (w * dx).sum(1), (w * dy).sum(1)
        if want_kl:
            kl = kl + (p * torch.log(p / q)).sum()
    return dY, Z, kl


def update_(dY, iY, gains, Y, mom):
    """gains, iY and Y in place; Y re-centred."""
    flip = (dY > 0) != (iY > 0)
    gains.copy_(torch.where(flip, gains + 0.2, gains * 0.8).clamp_(min=MIN_GAIN))
    iY.mul_(mom).sub_(ETA * (gains * dY))
    Y.add_(iY)
    Y.sub_(Y.mean(0, keepdim=True))


def iterate_(P, Y, iY, gains, first, last, kl_hist=None):
    """Iterations [first, last) in place; kl_hist[(it + 1) // 10 - 1] = KL when (it + 1) % 10 == 0."""
    for it in range(first, last):
        want = kl_hist is not None and (it + 1) % 10 == 0
        dY, _, kl = gradient(P, Y, exaggeration(it), want)
        update_(dY, iY, gains, Y, momentum(it))
        if want:
            kl_hist[(it + 1) // 10 - 1] = kl


def initial_embedding(n, seed):
    return torch.randn(n, 2, generator=torch.Generator().manual_seed(int(seed)))


# ---- the public entry ------------------------------------------------------------------------------------------------------------
def hip_applies(X, perplexity):
    """CUDA fp32 [N, D] with the switch on and a shape dts_supported takes; a missing library is an error here."""
    if not (_dbg.tsne_hip and X.is_cuda and X.dtype == torch.float32 and X.dim() == 2):
        return False
    from .. import _lib_tsne as lt
    return lt.supported(X.shape[0], X.shape[1], perplexity)


@torch.no_grad()
def tsne_exact(X, perplexity=30, n_iter=2000, seed=0):
    """(Y [N, 2], kl_history [n_iter // 10]) of X [N, D], in X's dtype and on its device."""
    assert X.dim() == 2 and X.is_floating_point(), "X must be a floating-point [N, D] tensor"
    N = X.shape[0]
    if not 0 < perplexity < N - 1:
        raise ValueError(f"perplexity {perplexity} must lie in (0, N - 1) for N = {N} points")
    X = pca(X.detach()).contiguous()
    Y = initial_embedding(N, seed).to(device=X.device, dtype=X.dtype)
    iY, gains = torch.zeros_like(Y), torch.ones_like(Y)
    kl_hist = X.new_zeros(max(int(n_iter) // 10, 0))
    if hip_applies(X, perplexity):
        from .. import _lib_tsne as lt
        plan = lt.plan(N)
        P, beta = X.new_empty((N, N)), X.new_empty(N)
        lt.cond_p(X, perplexity, P, beta)
        lt.symmetrize(P, X.new_empty(plan["sym_groups"]))
        lt.run(P, Y, iY, gains, torch.empty_like(Y), X.new_empty(plan["ws_floats"]), 0, int(n_iter), kl_hist if kl_hist.numel() else None)
    else:
        P, _ = cond_p(X, perplexity)
        symmetrize_(P)
        iterate_(P, Y, iY, gains, 0, int(n_iter), kl_hist)
    return Y, kl_hist


# ---- the reference's manager -----------------------------------------------------------------------------------------------------
class TsneManager:
    """utils/tsne_visualization.py TsneMAnager: per image, up to ``views_per_class`` pixels of every class that still lacks
    features; ``compute`` embeds what was gathered and writes the scatter plot."""

    def __init__(self, dataset, n_classes, feat_dim=None, run_id=None, scale=4, perplexity=30, iters=2000, feats_per_class=1000,
                 seed=0, experiment=1, palette=None):
        self.dataset = dataset
        self.n_classes = int(n_classes)
        self.feats_per_class = int(feats_per_class)
        self.feat_dim = feat_dim
        self.feats = []
        self.labels = []                                  # class id per row of the concatenated feats
        self.counts = [0] * self.n_classes
        self.scale = int(scale)
        self.run_id = run_id if run_id is not None else 'tsne'
        self.perplexity = perplexity
        self.iters = int(iters)
        self.seed = int(seed)
        self.experiment = experiment
        self.palette = palette
        self.generator = torch.Generator().manual_seed(self.seed)

    def views_per_class(self, cl):
        if self.dataset == 'CITYSCAPES' and cl >= 15:
            return 10
        return self.feats_per_class // 500

    def accumulate(self, feats, labels):
        n, h, w = labels.shape
        assert n == 1
        lbl_down = F.interpolate(labels.unsqueeze(1).float(), (h // self.scale, w // self.scale), mode='nearest').long().view(-1)
        assert feats.shape[0] == 1 and feats.shape[2] * feats.shape[3] == lbl_down.numel(), \
            f"features {list(feats.shape)} do not match the labels at stride {self.scale}: {[h // self.scale, w // self.scale]}"
        self.feat_dim = int(feats.shape[1])
        feats = feats[0].reshape(self.feat_dim, -1)
        for cl in range(self.n_classes):
            if self.counts[cl] >= self.feats_per_class:
                continue
            idx = (lbl_down == cl).nonzero().squeeze()
            if idx.dim() == 0:                            # exactly one pixel: the reference's squeeze() drops the class here
                continue
            take = min(self.views_per_class(cl), idx.shape[0])
            if take > 0:
                perm = torch.randperm(idx.shape[0], generator=self.generator)[:take].to(idx.device)
                self.feats.append(feats[:, idx[perm]].T.detach().float())
                self.labels += [cl] * take
                self.counts[cl] += take

    def file_stem(self):
        return f'{self.run_id}_perp-{self.perplexity}_its-{self.iters}_feats-per-class-{self.feats_per_class}_scale{self.scale}'

    def compute(self, log_dir):
        from .predict import class_palette
        if not self.feats:
            raise RuntimeError("TsneManager.compute: no features were accumulated")
        f = torch.cat(self.feats).contiguous()
        Y, kl = tsne_exact(f, self.perplexity, self.iters, self.seed)
        Y, kl = Y.cpu().numpy(), kl.cpu().numpy()
        labels = np.asarray(self.labels, dtype=np.int64)
        os.makedirs(str(log_dir), exist_ok=True)
        stem = os.path.join(str(log_dir), self.file_stem())
        colours = class_palette(self.dataset, self.experiment, self.palette).numpy()
        scatter_image(Y, labels, colours).save(stem + '.png')
        np.savez(stem + '.npz', Y=Y, labels=labels, kl=kl, counts=np.asarray(self.counts, dtype=np.int64))
        return Y


TsneMAnager = TsneManager                                 # the reference's spelling


def scatter_image(Y, labels, colours, size=1024, radius=3):
    """PIL image of the points Y [N, 2] as discs in ``colours[labels]`` on white, the axes scaled to the canvas."""
    from PIL import Image, ImageDraw
    img = Image.new('RGB', (size, size), (255, 255, 255))
    draw = ImageDraw.Draw(img)
    lo, hi = Y.min(0), Y.max(0)
    span = np.where(hi - lo > 0, hi - lo, 1.0)
    margin = 4 * radius
    xy = (Y - lo) / span * (size - 2 * margin) + margin
    for (x, y), cl in zip(xy, labels):
        x, y = float(x), float(size - y)
        draw.ellipse((x - radius, y - radius, x + radius, y + radius), fill=tuple(int(v) for v in colours[int(cl) % 256]))
    return img
