"""Generate the fixtures of the grounding input pipeline (runs where PIL and the reference tree are present):
  tests/golden/det_resize_*.npz   PIL `Image.resize((ow, oh), Image.BILINEAR)` -- what torchvision's F.resize does on a PIL image, the call of
                                  Resize.__call__ (fine_grained/maskrcnn_benchmark/data/transforms/transforms.py:118-128) -- of the seeded images of
                                  tests/det_input_cases.py: PIL's resized uint8 image and its shape
  tests/golden/det_boxes.npz      the reference's own BoxList.resize / BoxList.transpose(0) (structures/bounding_box.py, executed from the
                                  reference tree by path: it needs only torch) on the seeded boxes of det_input_cases.BOX_CASES
The fixtures hold arrays only.  python tools/gen_det_input_golden.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import shim                                      # noqa: E402
import det_input_cases as dc                                 # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def main():
    from PIL import Image
    for name, (H, W, oh, ow) in dc.RESIZE_CASES.items():
        r = np.asarray(Image.fromarray(dc.case_image(name), "RGB").resize((ow, oh), Image.BILINEAR))
        assert r.shape == (oh, ow, 3)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), resized=r, shape=np.array([H, W, oh, ow]))
        print("wrote", name, r.shape)
    bb = shim._load("bounding_box", os.path.join(shim.REF, "fine_grained", "maskrcnn_benchmark", "structures", "bounding_box.py"),
                    "maskrcnn_benchmark.structures")
    out = {}
    for name, (orig, new, flip) in dc.BOX_CASES.items():
        t = bb.BoxList(torch.from_numpy(dc.case_boxes(name)), orig, mode="xyxy").resize(new)
        if flip:
            t = t.transpose(bb.FLIP_LEFT_RIGHT)
        assert t.size == new and t.bbox.dtype == torch.float32
        out[name] = t.bbox.numpy()
    np.savez_compressed(os.path.join(OUT, dc.BOX_GOLDEN + ".npz"), **out)
    print("wrote", dc.BOX_GOLDEN, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
