"""Host side of the training image logs (model.py:968-1053 of the reference; the canvases themselves are rendered on the device,
csrc/canvas.hip): colour tables, file names, and the writer that turns pinned uint8 canvases into PNG files on one worker thread.

edflow's logging hook is absent from the reference tree.  What is restated here from memory is UNVERIFIED:
  * the file name  <root>/train/<name>_<step:07>.png;
  * the quantisation  uint8(clip((v + 1) * 127.5, 0, 255))  (truncating) that the colour tables below are put through on the host.
"""
import logging
import os
import queue
import threading

import numpy as np

LEVELS = (0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9)             # model.py:1009
LEVELS_TITLE = ("m0_sample_levels" + "-{}" * len(LEVELS)).format(*LEVELS).replace(".", "_")      # model.py:1018-1019
QUEUE_DEPTH = 2


def quantise_host(v):
    """float32 values -> bytes by the rule of the canvas kernels (fp64 arithmetic on the float32 values, truncation)."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    return np.clip((v + 1.0) * 127.5, 0.0, 255.0).astype(np.uint8)


def mask_colors01(n_parts):
    """nn.py:2118-2120: inferno at n_parts evenly spaced points, float64 [P,3] in [0,1]; a gray ramp without matplotlib (as
    model.mask_colors)."""
    try:
        from matplotlib import pyplot as plt
        return np.asarray(plt.cm.inferno(np.linspace(0, 1, n_parts))[:, :3], dtype=np.float64)
    except Exception:  # pragma: no cover
        return np.repeat(np.linspace(0, 1, n_parts)[:, None], 3, axis=1)


def mask_color_bytes(colors01):
    """nn.py:2075-2077: colours in [0,1] ([P,3], make_mask_colors) -> (c - 0.5) * 2 as float32 -> bytes [P,3]."""
    c = np.asarray(colors01, dtype=np.float64)
    return quantise_host(((c - 0.5) * 2).astype(np.float32))


def viridis_bytes():
    """nn.py:2060-2062: the 256 x 3 viridis table as float32, left in [0,1] as the reference leaves it -> bytes [256,3].  The table
    comes from matplotlib at run time; without matplotlib a gray ramp stands in (as model.mask_colors does)."""
    try:
        import matplotlib as mpl
        table = np.asarray(mpl.colormaps["viridis"].colors, dtype=np.float32)
    except Exception:  # pragma: no cover
        table = np.repeat(np.linspace(0, 1, 256, dtype=np.float32)[:, None], 3, axis=1)
    assert table.shape == (256, 3)
    return quantise_host(table)


def image_path(root, name, step):
    return os.path.join(root, "train", "{}_{:07d}.png".format(name, int(step)))


def have_pil():
    try:
        from PIL import Image  # noqa: F401
        return True
    except ImportError:
        return False


class Paletted(object):
    """A label map uint8 [H,W] with its palette uint8 [P,3]: ``encode_png`` writes it as a mode-P PNG -- viewers show the colours, the
    bytes are the labels (the segmentation export's label maps)."""

    def __init__(self, array, palette):
        self.array, self.palette = array, np.asarray(palette, dtype=np.uint8).reshape(-1, 3)


def encode_png(path, array):
    """uint8 [H,W,3] or [H,W,1] / [H,W] -> PNG, written under a temporary name and renamed.  A ``Paletted`` map -> a palette PNG."""
    from PIL import Image
    palette = None
    if isinstance(array, Paletted):
        array, palette = array.array, array.palette
    a = np.asarray(array)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    tmp = path + ".tmp-{}".format(os.getpid())
    if palette is None:
        img = Image.fromarray(a)
    else:
        img = Image.fromarray(np.ascontiguousarray(a, dtype=np.uint8), mode="P")
        img.putpalette(palette.tobytes())
    img.save(tmp, format="PNG")
    os.replace(tmp, path)


class ImageWriter(object):
    """One worker thread behind a bounded queue (depth 2).  ``submit`` hands over the canvases of one step -- host arrays, or pinned
    tensors with the event of the copy that fills them -- and BLOCKS while the queue is full: nothing is ever dropped.  ``flush``
    returns once everything submitted has been written; ``close`` also ends the thread.  An exception in the worker is re-raised by
    the next submit / flush / close.  ``path_fn(root, name, step)`` names the files (default: ``image_path``, the training logs'
    rule); the file's directory is created."""

    def __init__(self, root, encode=encode_png, depth=QUEUE_DEPTH, path_fn=image_path):
        self.root, self.encode, self.path_fn = root, encode, path_fn
        self.q = queue.Queue(maxsize=depth)
        self.error = None
        self.written = []
        self.thread = threading.Thread(target=self._work, name="upsparts-image-writer", daemon=True)
        self.thread.start()

    def _work(self):
        while True:
            item = self.q.get()
            try:
                if item is None:
                    return
                step, images, ready = item
                if self.error is None:
                    if ready is not None:
                        ready.synchronize()                     # the device-to-host copies of this step (side stream)
                    if self.path_fn is image_path:
                        os.makedirs(os.path.join(self.root, "train"), exist_ok=True)
                    for name, a in images.items():
                        path = self.path_fn(self.root, name, step)
                        os.makedirs(os.path.dirname(path), exist_ok=True)
                        self.encode(path, a.numpy() if hasattr(a, "numpy") else a)
                        self.written.append(path)
            except BaseException as e:      # noqa: B902 -- reported to the training thread
                self.error = e
            finally:
                self.q.task_done()

    def _raise(self):
        if self.error is not None:
            e, self.error = self.error, None
            raise e

    def submit(self, step, images, ready=None):
        self._raise()
        self.q.put((step, images, ready))                       # blocks while two steps are waiting

    def flush(self):
        self.q.join()
        self._raise()

    def close(self):
        if self.thread.is_alive():
            self.q.put(None)
            self.thread.join()
        self._raise()


_warned = set()


def warn_once(logger, key, msg):
    if key in _warned:
        return
    _warned.add(key)
    (logger or logging.getLogger("upsparts")).warning(msg)
