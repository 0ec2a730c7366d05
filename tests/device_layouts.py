"""Layouts of a caller's device frames for tests/test_device_layouts_gpu.py: a batch of frames packed into one byte buffer at any base
offset, row step and frame gap, every byte that is no pixel set to a fill.  Plain numpy; the device copy goes through the library's
own allocator (tests/pose_opt_device.py)."""
import numpy as np

RANDOM = "random"      # fill: seeded random bytes
TAIL = 64              # bytes behind the last frame's last full step: an over-read of slack stays inside the allocation


def align_up(v, a):
    return (v + a - 1) // a * a


def layouts(cols):
    """(name, base_off, step, frame_gap) of every layout the device-pointer tests run."""
    return [
        ("tight", 0, cols, 0),
        ("control", 0, align_up(cols, 64) + 64, 0),                 # 64-byte rows: what the host-pointer staging hands the kernels
        ("odd", 1, cols + 1, 3),                                    # every row at another residue mod 4, 8 and 16
        ("mod4", 4, cols + 4, 4),                                   # aligned to 4, not to 8
        ("mod8", 8, cols + 8, 8),                                   # aligned to 8, not to 16
        ("step8", 0, (cols // 8 + 1) * 8, 0),                       # the next multiple of 8 strictly above cols
    ]


def frame_stride(rows, step, frame_gap):
    return rows * step + frame_gap


def nbytes(B, rows, base_off, step, frame_gap):
    return base_off + (B - 1) * frame_stride(rows, step, frame_gap) + rows * step + TAIL


def pixel_mask(B, rows, cols, base_off, step, frame_gap):
    """bool per byte of the packed buffer: is it a pixel?"""
    m = np.zeros(nbytes(B, rows, base_off, step, frame_gap), bool)
    view(m, B, rows, cols, base_off, step, frame_gap)[...] = True
    return m


def view(buf, B, rows, cols, base_off, step, frame_gap):
    """The (B, rows, cols) strided view of the frames inside a packed buffer (no copy)."""
    assert buf.ndim == 1 and buf.itemsize == 1 and step >= cols
    return np.lib.stride_tricks.as_strided(buf[base_off:], (B, rows, cols), (frame_stride(rows, step, frame_gap), step, 1))


def pack(frames, base_off, step, frame_gap, fill, seed=0):
    """frames (B, rows, cols) uint8 -> one uint8 buffer: frame f's row y starts at base_off + f * (rows * step + frame_gap) + y * step.
    Every other byte -- in front of the base, behind a row's pixels, between frames, the TAIL -- is `fill`: a byte value, or RANDOM
    (bytes from a generator seeded with `seed`)."""
    frames = np.asarray(frames, np.uint8)
    B, rows, cols = frames.shape
    n = nbytes(B, rows, base_off, step, frame_gap)
    if isinstance(fill, str):
        assert fill == RANDOM
        buf = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    else:
        buf = np.full(n, fill, np.uint8)
    view(buf, B, rows, cols, base_off, step, frame_gap)[...] = frames
    return buf
