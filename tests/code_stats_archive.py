"""The small archive tests/test_code_stats_cpu.py and tests/test_code_stats_gpu.py both count."""
import numpy as np


def small_archive(path, with_all_masks=True):
    """two normal_*, two tumor_*, two test_* slides of unequal sizes, uint8 and uint16 codes below 300"""
    from vqae_amd import hdf5
    rng = np.random.RandomState(5)
    images, masks = {}, {}
    shapes = {"normal_001": (5, 9), "normal_002": (16, 16), "tumor_001": (7, 33), "tumor_002": (12, 5), "test_001": (9, 9),
              "test_002": (3, 40)}
    for i, (stem, shp) in enumerate(shapes.items()):
        wide = i % 2 == 1
        images[stem] = rng.randint(0, 300 if wide else 200, shp).astype(np.uint16 if wide else np.uint8)
        m = rng.randint(0, 2, shp)
        if "normal" not in stem:
            m[rng.rand(*shp) < 0.2] = 2
        masks[stem + "_mask"] = m.astype(np.uint8)
    if not with_all_masks:
        del masks["tumor_002_mask"]
    hdf5.write_hdf5(str(path), {"images": images, "masks": masks})
    return images, masks
