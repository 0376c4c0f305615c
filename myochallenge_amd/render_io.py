"""Host-side helpers of the renderer: a PNG writer on the standard library (zlib) and SB3's image tiling."""
from __future__ import annotations

import struct
import zlib
from typing import Sequence

import numpy as np


def png_bytes(img: np.ndarray) -> bytes:
    """8-bit RGB (H, W, 3) or grey (H, W) image -> PNG file contents (one IDAT chunk, filter 0 on every row)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError("png_bytes takes an (H, W, 3) or (H, W) uint8 image")
    h, w = img.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, -1)], axis=1).tobytes()

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if img.ndim == 3 else 0, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")


def write_png(path: str, img: np.ndarray) -> None:
    with open(path, "wb") as f:
        f.write(png_bytes(img))


def tile_images(images: Sequence[np.ndarray]) -> np.ndarray:
    """stable_baselines3.common.vec_env.base_vec_env.tile_images: N images of (H, W, C) -> one grid of ceil(sqrt(N)) columns, the
    missing cells black."""
    imgs = np.asarray(images)
    n, h, w, c = imgs.shape
    cols = int(np.ceil(np.sqrt(n)))
    rows = int(np.ceil(n / cols))
    imgs = np.concatenate([imgs, np.zeros((rows * cols - n, h, w, c), imgs.dtype)], axis=0)
    return imgs.reshape(rows, cols, h, w, c).transpose(0, 2, 1, 3, 4).reshape(rows * h, cols * w, c)
