"""Inputs for the batched stereo matchers (plain NumPy, no GPU): stacks of B different pairs whose
content next to the seams between image b and image b + 1 would show a batch kernel that reads or
joins across a seam.  tests/test_stereo_batch_inputs.py (CPU) shows with the restatements alone that
each stack can catch such a leak: matched as ONE tall image, the rows next to the seams come out
different from the per-image results.  tests/test_gpu_stereo_batch.py holds the GPU to the per-image
results, bit for bit."""
import numpy as np

import bm_reference as B
import sgbm_reference as R
import stereo_inputs as SI

# the smallest shapes at which a batch can go wrong: an odd width, rows no multiple of anything
SHAPES = ((80, 48, 16), (97, 50, 32))   # (W, H, num_disparities)
NB = 3


def params(matcher, D, speckle_window_size):
    """The reference's defaults at D disparities; BM with a block and a uniqueness ratio that leave
    something valid at these widths (the defaults' 15 / 80 filter nearly every pixel of noise)."""
    if matcher == "sgbm":
        return R.Params(num_disparities=D, speckle_window_size=speckle_window_size)
    return B.Params(num_disparities=D, speckle_window_size=speckle_window_size, block_size=7,
                    uniqueness_ratio=15)


def noise_stack(W, H, kind="half", nb=NB):
    """nb pairs of different seeds: the vertical cost sums, the SGBM chains and BM's window sums of one
    image continued into the next would see other values."""
    fam = SI.half_correlated if kind == "half" else SI.uncorrelated_noise
    kw = dict(k=5) if kind == "half" else {}
    pairs = [fam(H, W, seed=11 + 7 * b, **kw) for b in range(nb)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


SPECKLE_D0, SPECKLE_STEP = 2, 8


def speckle_stack(W, H, nb=NB):
    """SGBM: a textured ground at disparity 2 (one large region) and, at every seam, a patch of 7 x 14
    pixels at disparity 10 on the bottom rows of image b and another on the top rows of image b + 1,
    in the same columns.  Each is a region well below speckle_window_size = 100 and is removed; joined
    across the seam they would exceed it and stay.  (BM never labels the rows next to a seam: its
    matched region ends block_size / 2 rows inside the image, so its regions cannot meet there.)"""
    rng = np.random.default_rng(5)
    lefts, rights = [], []
    x0, pw, ph = W - 30, 14, 7
    for b in range(nb):
        left, right = SI._shifted(rng.integers(0, 256, (H, W + SPECKLE_D0), dtype=np.uint8), W, SPECKLE_D0)
        for y0 in ([H - ph] if b < nb - 1 else []) + ([0] if b > 0 else []):
            tex = rng.integers(0, 256, (ph, pw), dtype=np.uint8)
            d = SPECKLE_D0 + SPECKLE_STEP
            left[y0:y0 + ph, x0:x0 + pw] = tex
            right[y0:y0 + ph, x0 - d:x0 - d + pw] = tex
        lefts.append(left)
        rights.append(right)
    return np.stack(lefts), np.stack(rights)


def restate_each(matcher, lefts, rights, p, masks=None):
    M = R if matcher == "sgbm" else B
    outs = [M.restate(lefts[b], rights[b], p, None if masks is None else masks[b])
            for b in range(lefts.shape[0])]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def restate_tall(matcher, lefts, rights, p):
    """The same images matched as ONE image of nb * H rows: what a kernel without seams would give."""
    M = R if matcher == "sgbm" else B
    nb, H, W = lefts.shape
    f, raw = M.restate(lefts.reshape(nb * H, W), rights.reshape(nb * H, W), p, None)
    return f.reshape(nb, H, W), raw.reshape(nb, H, W)


def seam_rows(H, nb, reach):
    """Boolean (nb, H): rows within `reach` rows of a seam between two images."""
    m = np.zeros((nb, H), bool)
    m[:-1, H - reach:] = True
    m[1:, :reach] = True
    return m


_chains = {}


def cpu_chain(seq, pairs, use_bm, frames=None, key=None, floor=0.25):
    """tests/stereo_sequence.py's cpu_chain (the same pieces, through its cpu_pair) for the small
    frames of the batch tests.  At 160 x 120 and the reference's 80 disparities only W - 81 = 79 of
    160 columns can match at all (49 %), so that module's floor of 40 % of W x H points per pair is
    out of reach here; the floor of these tests is half of what can match: 25 %."""
    import stereo_sequence as SS
    if key is not None and key in _chains:
        return _chains[key]
    xs, is_, ns, last = [], [], [], None
    for (i, j) in pairs:
        x, it, last = SS.cpu_pair(seq, i, j, use_bm, frames=frames)
        assert x.shape[0] > floor * seq.W * seq.H, (i, j, x.shape[0] / float(seq.W * seq.H))
        xs.append(x)
        is_.append(it)
        ns.append(x.shape[0])
    out = (np.concatenate(xs), np.concatenate(is_), ns, last)
    if key is not None:
        _chains[key] = out
    return out
