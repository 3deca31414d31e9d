"""What the CPU and GPU tests of vrt_scene_morph share: the volumes.  Volumes are uint8 arrays indexed [z, y, x]."""
import numpy as np


def blobs(dims, seed, p=0.5, block=3, speckle=0.04, holes_only=False):
    """a volume of coarse random blocks with speckle: solids thick enough to survive an erosion, holes small enough to close.
    holes_only: the speckle only punches holes, so an empty block stays empty (block = 8: an absent brick)"""
    W, H, D = dims
    rng = np.random.default_rng(seed)
    coarse = rng.random((-(-D // block), -(-H // block), -(-W // block))) < p
    vol = np.repeat(np.repeat(np.repeat(coarse, block, 0), block, 1), block, 2)[:D, :H, :W]
    noise = rng.random((D, H, W)) < speckle
    vol = (vol & ~noise) if holes_only else (vol ^ noise)
    return (vol * rng.integers(1, 199, (D, H, W))).astype(np.uint8)
