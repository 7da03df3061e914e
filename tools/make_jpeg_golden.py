"""Writes tests/golden/jpeg_cases.npz: JPEG files and the pixels PIL (libjpeg-turbo) decodes them to, as BGR -- the yardstick of
siammask_amd.jpeg.  Needs PIL.

    python tools/make_jpeg_golden.py --tennis <folder with 00000.jpg and 00001.jpg of the tennis sequence>

Cases = sizes x contents x encodings (7 x 2 x 8 = 112): the smallest shapes at which partial MCUs on both axes, odd chroma widths,
a one-MCU image, one-MCU restart segments and every table path occur.  Also: the two tennis frames as bytes with the sha256 of
their pixels and a 64 x 64 crop for diagnosis, one progressive and one CMYK file for the refusals.
"""
import argparse
import hashlib
import io
import os

import numpy as np
from PIL import Image

SIZES = [(8, 8), (16, 16), (17, 23), (1, 1), (9, 33), (31, 15), (40, 72)]
CONTENTS = ("noise", "smooth")
ENCODINGS = [("444_q80", dict(subsampling=0, quality=80)), ("422_q80", dict(subsampling=1, quality=80)),
             ("420_q80", dict(subsampling=2, quality=80)), ("420_rst1", dict(subsampling=2, quality=80, restart_marker_blocks=1)),
             ("420_opt_q30", dict(subsampling=2, optimize=True, quality=30)), ("444_q100", dict(subsampling=0, quality=100)),
             ("420_q5", dict(subsampling=2, quality=5)), ("grey_q85", None)]
CROP = (200, 400)                                                     # (y, x) of the tennis crops


def image(rs, h, w, kind):
    if kind == "noise":
        return (rs.rand(h, w, 3) * 255).astype(np.uint8)
    yy, xx = np.mgrid[:h, :w]
    a = np.stack([(xx * 7 + yy * 3) % 256, (xx * 2 + yy * 11) % 256, (xx * yy) % 256], -1).astype(np.uint8)
    a[h // 3:h // 2 + 1, w // 4:w // 2 + 1] = [255, 0, 0]             # a saturated rectangle
    return a


def pil_bgr(b):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))[:, :, ::-1])


def cases():
    rs = np.random.RandomState(1)
    for h, w in SIZES:
        for kind in CONTENTS:
            for name, kw in ENCODINGS:
                a, bio = image(rs, h, w, kind), io.BytesIO()
                if kw is None:
                    Image.fromarray(a[:, :, 0]).save(bio, "JPEG", quality=85)
                else:
                    Image.fromarray(a).save(bio, "JPEG", **kw)
                yield "%dx%d_%s_%s" % (h, w, kind, name), bio.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tennis", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_cases.npz"))
    a = ap.parse_args()
    names, files, pix = [], [], []
    for name, b in cases():
        names.append(name)
        files.append(np.frombuffer(b, dtype=np.uint8))
        pix.append(pil_bgr(b))
    d = {"names": np.asarray(names), "hw": np.asarray([p.shape[:2] for p in pix], dtype=np.int32),
         "file_off": np.concatenate([[0], np.cumsum([f.size for f in files])]).astype(np.int64), "files": np.concatenate(files),
         "pix_off": np.concatenate([[0], np.cumsum([p.size for p in pix])]).astype(np.int64), "pix": np.concatenate([p.reshape(-1) for p in pix])}
    sha, crops = [], []
    for k, f in enumerate(("00000.jpg", "00001.jpg")):
        b = open(os.path.join(a.tennis, f), "rb").read()
        p = pil_bgr(b)
        d["tennis%d" % k] = np.frombuffer(b, dtype=np.uint8)
        sha.append(hashlib.sha256(p.tobytes()).hexdigest())
        crops.append(p[CROP[0]:CROP[0] + 64, CROP[1]:CROP[1] + 64])
    d["tennis_hw"], d["tennis_sha256"], d["tennis_crop"], d["tennis_crop_yx"] = np.asarray(p.shape[:2]), np.asarray(sha), np.stack(crops), np.asarray(CROP)
    rs = np.random.RandomState(2)
    bio = io.BytesIO()
    Image.fromarray(image(rs, 24, 24, "smooth")).save(bio, "JPEG", progressive=True)
    d["progressive"] = np.frombuffer(bio.getvalue(), dtype=np.uint8)
    bio = io.BytesIO()
    Image.fromarray(image(rs, 16, 16, "noise")).convert("CMYK").save(bio, "JPEG")
    d["cmyk"] = np.frombuffer(bio.getvalue(), dtype=np.uint8)
    np.savez(a.out, **d)
    print(a.out, os.path.getsize(a.out), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
