"""Host side of the training image logs (no GPU): the tiling arithmetic of the fp64 restatement (tests/imglog_ref.py), the image-step
cadence of ``Trainer.iterate``, the file names, the writer's bounded queue, and that header, binding and library agree on the
ups_canvas_* entry points."""
import os
import re
import threading

import numpy as np
import pytest
import torch

import imglog_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANVAS = ("ups_canvas_grid_side", "ups_canvas_images", "ups_canvas_mask_rgb", "ups_canvas_assigned_parts", "ups_canvas_first_item")


def _pkg():
    import upsparts_amd  # noqa: F401
    from upsparts_amd import imglog, lib, model, ops
    return imglog, lib, model, ops


def test_tiling_arithmetic():
    assert IR.canvas_grid(5) == (3, 3) and IR.canvas_grid(7, 5) == (2, 5) and IR.canvas_grid(1) == (1, 1)
    assert IR.canvas_grid(4) == (2, 2) and IR.canvas_grid(9) == (3, 3) and IR.canvas_grid(10) == (4, 4) and IR.canvas_grid(10, 5) == (2, 5)
    x = np.arange(1, 6, dtype=np.float64)[:, None, None, None] * np.ones((5, 2, 3, 1))
    c = IR.batch_to_canvas(x)
    assert c.shape == (3 * 2, 3 * 3, 1)
    tiles = [c[r * 2:(r + 1) * 2, q * 3:(q + 1) * 3, 0] for r in range(3) for q in range(3)]
    assert [float(t[0, 0]) for t in tiles] == [1, 2, 3, 4, 5, 0, 0, 0, 0] and all((t == t[0, 0]).all() for t in tiles)
    assert sum(bool((t == 0).all()) for t in tiles) == 4                        # 4 blank tiles, value 0 ...
    assert (IR.quantise(c)[2 * 2:, :, 0] == 127).all()                          # ... byte 127
    assert IR.batch_to_canvas(np.ones((7, 2, 3, 3)), 5).shape == (2 * 2, 5 * 3, 3)
    one = np.random.RandomState(0).uniform(-1, 1, (1, 4, 4, 3))
    assert np.array_equal(IR.batch_to_canvas(one), one[0]) and IR.plot_batch(one).shape == (4, 4, 3)
    # the quantisation: truncation, both clamps, 0 -> 127, 1 -> 255
    assert IR.quantise(np.array([-1.5, -1.0, 0.0, 1.0, 1.5, -1 + 0.5 / 127.5, -1 + 1.5 / 127.5])).tolist() == [0, 0, 127, 255, 255, 0, 1]


def test_grid_side_of_the_library():
    _, lib, _, ops = _pkg()
    h = lib.load()
    for n in list(range(1, 70)) + [128, 1 << 20, (1 << 20) + 1]:
        g = h.ups_canvas_grid_side(n)
        assert (g - 1) ** 2 < n <= g * g and (g, g) == IR.canvas_grid(n) == ops.canvas_grid(n)
    assert ops.canvas_grid(7, 5) == IR.canvas_grid(7, 5) == (2, 5)


def test_assigned_parts_shape():
    B, S, P = 3, 16, 7
    rng = np.random.RandomState(1)
    hard = np.eye(P)[rng.randint(0, P, (2, B, S, S))]
    views = rng.uniform(-1, 1, (2, B, S, S, 3))
    assert IR.canvas_grid(2 * B) == (3, 3) and IR.canvas_grid(P, 5) == (2, 5)
    c = IR.assigned_parts(hard[0], hard[1], views[0], views[1])
    assert c.shape == (2 * 3 * S, 5 * 3 * S, 3) and c.dtype == np.uint8
    g = 3 * S
    # part 6 sits in grid (1, 1); its tile 4 (row 1, column 1 of the inner grid) is image 1 of view 1 under the encoding mask
    tile = c[g + S:g + 2 * S, g + S:g + 2 * S]
    assert np.array_equal(tile, IR.quantise(hard[1][1][..., 6:7] * views[1][1]))
    assert (c[g:, 2 * g:] == 127).all()                                        # grids 7, 8, 9 of the outer canvas are blank
    assert (c[2 * S:g, :] == 127).all()                                        # inner tiles 6, 7, 8 of the upper grids as well


class _StubTrainer(object):
    """Trainer.iterate on a trainer whose step does nothing: records which steps log scalars and which ask for images."""

    def __init__(self, model_mod, log_images, log_freq):
        self.config = {"log_freq": log_freq, "ckpt_freq": 100}
        self.global_step, self.root, self.rank, self.world_size, self.process_group = 0, None, 0, 1, None
        self.device, self.switches_report, self.log_images = torch.device("cpu"), "stub", log_images
        self.scalar_steps, self.image_steps, self.written, self.events = [], [], [], []
        self._iterate = model_mod.Trainer.iterate

    def train_step(self, batch, noise=None, images=False):
        if images:
            self.image_steps.append(self.global_step)
        self.global_step += 1

    def fetch_logs(self):
        self.scalar_steps.append(self.global_step - 1)
        return {"loss_x": 0.0}

    def _write_images(self, step):
        self.written.append(step)

    def _flush_images(self, close=False):
        self.events.append(("flush", close, self.global_step))

    def _checkpoint(self):
        self.events.append(("checkpoint", None, self.global_step))


@pytest.mark.parametrize("log_freq", [250, 40])
def test_image_steps_are_the_scalar_log_steps(log_freq):
    _, _, M, _ = _pkg()
    on, off = _StubTrainer(M, True, log_freq), _StubTrainer(M, False, log_freq)
    for t in (on, off):
        t._iterate(t, iter(lambda: {}, None), num_steps=600, log_fn=lambda line: None)
    want = {250: [0, 2, 4, 8, 16, 32, 64, 128, 250, 500], 40: [0, 2, 4, 8, 16, 32] + list(range(40, 600, 40))}[log_freq]
    assert on.scalar_steps == want
    assert on.image_steps == on.written == on.scalar_steps == off.scalar_steps
    assert off.image_steps == [] and off.written == []
    # every checkpoint is preceded by a flush of the writer, and the loop ends with the writer closed
    for t in (on, off):
        for i, ev in enumerate(t.events):
            if ev[0] == "checkpoint":
                assert t.events[i - 1][0] == "flush" and t.events[i - 1][2] == ev[2]
        assert t.events[-2] == ("flush", True, 600) and t.events[-1] == ("checkpoint", None, 600)


def test_file_names():
    IL, _, _, _ = _pkg()
    assert IL.image_path("/r", "generated", 0) == os.path.join("/r", "train", "generated_0000000.png")
    assert IL.image_path("/r", "view0", 1250) == os.path.join("/r", "train", "view0_0001250.png")
    assert IL.LEVELS_TITLE == IR.LEVELS_TITLE == "m0_sample_levels-0_01-0_05-0_1-0_25-0_5-0_75-0_9"
    assert IL.LEVELS == IR.P_LEVELS


def test_host_colour_tables():
    IL, _, _, _ = _pkg()
    pytest.importorskip("matplotlib")
    for P in (3, 10, 25):
        assert np.array_equal(IL.mask_color_bytes(IL.mask_colors01(P)), IR.quantise(IR.mask_colors(P)))
    v = IL.viridis_bytes()
    assert v.shape == (256, 3) and v.dtype == np.uint8 and np.array_equal(v, IR.quantise(IR.viridis()))
    assert v.min() >= 127                                                       # a table in [0,1]: gray to white


def test_writer_queue_blocks_and_never_drops(tmp_path):
    """With the worker held inside an encode and two steps queued, a further submit must BLOCK: it reaches queue.Queue.put on a
    full queue of depth 2 with block=True and no timeout (observed at the call, so the test does not have to wait on a blocked
    thread).  Once the worker is released every submitted step is written, in order."""
    import queue
    IL, _, _, _ = _pkg()
    gate, started, seen = threading.Event(), threading.Event(), []

    def encode(path, a):
        started.set()
        assert gate.wait(30)
        seen.append((os.path.basename(path), int(a[0, 0, 0])))

    w = IL.ImageWriter(str(tmp_path), encode=encode)
    assert IL.QUEUE_DEPTH == 2 and w.q.maxsize == 2
    img = lambda i: {"generated": np.full((2, 2, 3), i, dtype=np.uint8)}
    w.submit(0, img(0))
    assert started.wait(30)             # the worker holds step 0 and waits inside encode: the queue is empty again
    w.submit(1, img(1))
    w.submit(2, img(2))
    assert w.q.full() and seen == []
    put, calls = w.q.put, []

    class WouldBlock(Exception):
        pass

    def observed_put(item, block=True, timeout=None):
        calls.append((block, timeout, w.q.full()))
        if w.q.full():
            raise WouldBlock()
        return put(item, block, timeout)
    w.q.put = observed_put
    with pytest.raises(WouldBlock):
        w.submit(3, img(3))
    assert calls == [(True, None, True)], "submit on a full queue must be a blocking put without a timeout"
    w.q.put = put
    with pytest.raises(queue.Full):
        w.q.put_nowait(None)            # (the queue itself is bounded)
    gate.set()
    w.submit(3, img(3))                 # blocks until the worker has taken step 1
    w.close()
    assert seen == [("generated_{:07d}.png".format(i), i) for i in range(4)]
    assert not w.thread.is_alive() and os.path.isdir(str(tmp_path / "train"))


def test_writer_reports_a_failed_encode(tmp_path):
    IL, _, _, _ = _pkg()

    def encode(path, a):
        raise OSError("disk full")
    w = IL.ImageWriter(str(tmp_path), encode=encode)
    w.submit(0, {"x": np.zeros((1, 1, 3), np.uint8)})
    with pytest.raises(OSError):
        w.flush()
    w.close()


def test_png_round_trip(tmp_path):
    IL, _, _, _ = _pkg()
    pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.RandomState(0)
    rgb, gray = rng.randint(0, 256, (6, 5, 3), dtype=np.uint8), rng.randint(0, 256, (6, 5, 1), dtype=np.uint8)
    w = IL.ImageWriter(str(tmp_path))
    w.submit(7, {"a": rgb, "b": gray})
    w.close()
    assert np.array_equal(np.asarray(Image.open(IL.image_path(str(tmp_path), "a", 7))), rgb)
    assert np.array_equal(np.asarray(Image.open(IL.image_path(str(tmp_path), "b", 7))), gray[:, :, 0])
    assert sorted(os.listdir(str(tmp_path / "train"))) == ["a_0000007.png", "b_0000007.png"]


def test_canvas_symbols_in_header_binding_and_library():
    _, lib, _, _ = _pkg()
    hdr = open(os.path.join(ROOT, "include", "upsparts_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(ups_canvas_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(CANVAS) == {n for n in lib.EXPORTS if n.startswith("ups_canvas_")}
    handle = lib.load()
    for name in CANVAS:
        fn = getattr(handle, name)
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(fn.argtypes) == len([a for a in args.split(",") if a.strip()]), name
    flags = open(os.path.join(ROOT, "unsupervised-part-segmentation_amd", "csrc", "flags.sh")).read()
    assert "canvas" in re.search(r'UPS_SOURCES="([^"]*)"', flags).group(1).split()


def test_log_images_defaults_to_off():
    _, _, M, _ = _pkg()
    import inspect
    src = inspect.getsource(M.Trainer.__init__)
    assert 'config.get("log_images", False)' in src
