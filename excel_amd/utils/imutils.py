"""Host-side format helpers either side of the path: mirror of the live parts of utils/imutils.py and of the on-disk
records tools/infer_lam.py exchanges with its CRF stage.

  colormap / encode_cmap   utils/imutils.py:7-9, :32-50   (the PASCAL VOC palette: bit-interleaved class index)
  save_logits/load_logits  tools/infer_lam.py:116-119 (writer), :203-206 (reader): np.save of the dict
                           {"valid_lam": cams [k+1,H,W] f32, "keys_gt": present classes int64}
  crf_keys_to_labels       tools/infer_lam.py:225-227: keys = pad(keys_gt + 1, (1, 0)); label = keys[argmax]
  save_label_png           the colour-coded label image the reference writes with imageio (:228); PIL here
  voc_test_palette / convert_test_seg2RGB   utils/pyutils.py:183-217: the VOC test-server palette PNG (21 VOC colours, grey after)
  jet_lut / denormalize_roundtrip_table / cam_overlay_tables / CamOverlayWriter
                           tools/infer_lam.py:97-111 (--save_cam): the host half of the CAM overlay images (the blend itself is
                           excel_cam_overlay_ragged, camviz.hip)
  CamJpegWriter            tools/infer_lam.py:104,111 (--save_cam --cam_device_jpeg true): the host half of the device-encoded overlay files
                           (excel_jpeg_encode_rgb_ragged, jpeg.hip)
  LabelPngWriter           tools/infer_lam.py:95 / tools/training_free_attr.py:225 (--save_label): the host half of the label PNG files
                           (the files themselves are encoded by excel_png_encode_labels_ragged, png.hip)

Plain numpy / PIL on the host: these are file formats, not compute.  DenseCRF itself (utils/dcrf.py) is excel_amd/utils/dcrf.py over
excel_dcrf_inference (crf.hip).
"""
import os

import numpy as np


def colormap(N=256, normalized=False):
    """VOC palette: colour channel bits are the class index's bits taken 3 at a time, MSB first (imutils.py:32-50)."""
    idx = np.arange(N, dtype=np.int64)
    cmap = np.zeros((N, 3), dtype=np.int64)
    c = idx.copy()
    for j in range(8):
        for ch in range(3):
            cmap[:, ch] |= ((c >> ch) & 1) << (7 - j)
        c >>= 3
    return (cmap / 255).astype(np.float32) if normalized else cmap.astype(np.uint8)


def encode_cmap(label):
    """label [H,W] (any integer dtype; 255 = ignore -> white-ish palette entry) -> RGB uint8 [H,W,3] (imutils.py:7-9)."""
    return colormap()[np.asarray(label).astype(np.int16), :]


def denormalize_img(imgs=None, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
    """utils/imutils.py:11-19 (device tensor in, uint8 device tensor out; HIP kernel)."""
    from .. import ops
    return ops.denormalize_img(imgs, mean, std, as_float=False)


def denormalize_img2(imgs=None):
    """utils/imutils.py:21-25: denormalize_img(imgs) / 255.0 (the PAR guide image of the training loop, scripts/train_voc.py:181)."""
    from .. import ops
    return ops.denormalize_img(imgs, as_float=True)


def save_logits(logits_dir, name, valid_lam, keys_gt, run_token=None):
    """tools/infer_lam.py:116-119.  `run_token` (optional, an extra key next to the reference's two: its reader looks keys up by name)
    marks the run that wrote the record, so the CRF stage can refuse records of an earlier run whatever the file system's time
    stamps say."""
    os.makedirs(logits_dir, exist_ok=True)
    valid_lam = valid_lam.detach().cpu().numpy() if hasattr(valid_lam, "detach") else np.asarray(valid_lam)
    keys_gt = keys_gt.detach().cpu().numpy() if hasattr(keys_gt, "detach") else np.asarray(keys_gt)
    path = os.path.join(logits_dir, name + ".npy")
    rec = {"valid_lam": valid_lam, "keys_gt": keys_gt}
    if run_token is not None:
        rec["run_token"] = str(run_token)
    np.save(path, rec)
    return path


def logits_run_token(path):
    """The run token of a record written by save_logits (None: written without one, e.g. by the reference)."""
    return np.load(path, allow_pickle=True).item().get("run_token")


def load_logits(path):
    """tools/infer_lam.py:203-206 -> (valid_lam, keys_gt)."""
    d = np.load(path, allow_pickle=True).item()
    return d["valid_lam"], d["keys_gt"]


def crf_keys_to_labels(prob, keys_gt):
    """tools/infer_lam.py:225-227: prob [k+1,H,W] -> uint8 labels through keys = [0, keys_gt + 1...]."""
    pred = np.argmax(prob, axis=0)
    keys = np.pad(np.asarray(keys_gt) + 1, (1, 0), mode="constant")
    return keys[pred].astype(np.uint8)


def save_label_png(path, label):
    """Colour-coded label image (tools/infer_lam.py:228)."""
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(encode_cmap(np.squeeze(label)).astype(np.uint8)).save(path)
    return path


def voc_test_palette():
    """The palette of utils/pyutils.py:183-217 (convert_test_seg2RGB), 256 x 3 uint8: index i is grey (i, i, i), except the first 21
    entries, which are the VOC class colours (colormap()[:21])."""
    pal = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    pal[:21] = colormap(21)
    return pal


def convert_test_seg2RGB(label, path):
    """utils/pyutils.py:183-217: uint8 labels [H,W] -> a palette ("P" mode) PNG at `path`, the format of the VOC test server's
    results/VOC2012/Segmentation/comp6_test_cls/<name>.png."""
    from PIL import Image
    im = Image.fromarray(np.asarray(label).astype(np.uint8))
    im.putpalette(voc_test_palette().reshape(-1).tolist())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    im.save(path)
    return path


# ------------------------------------------------------------------ CAM overlay images (tools/infer_lam.py:97-111)
# matplotlib's "jet" (_cm.py _jet_data): (x, y0, y1) anchors per channel.  matplotlib is not a dependency: the table is restated here.
JET_SEGMENTS = {
    "red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
    "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
    "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
}
CAM_ALPHA_MAX = 0.5          # :101, the max-over-classes overlay
CAM_ALPHA_PER_CLASS = 0.6    # :108, one overlay per present class
CAM_JPEG_QUALITY = 75        # imageio's Pillow writer (and Pillow) default


def _segment_lut(N, data):
    """LinearSegmentedColormap._create_lookup_table(N, data, gamma=1.0), float64 [N]."""
    a = np.array(data, np.float64)
    x, y0, y1 = a[:, 0] * (N - 1), a[:, 1], a[:, 2]
    xind = (N - 1) * np.linspace(0, 1, N) ** 1.0
    ind = np.searchsorted(x, xind)[1:-1]
    distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.concatenate([[y1[0]], distance * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
    return np.clip(lut, 0.0, 1.0)


def jet_lut(N=256):
    """matplotlib's jet colormap table, float64 [N,3] (RGB; what plt.get_cmap("jet")(x)[..., :3] reads for 0 <= x <= 1)."""
    return np.stack([_segment_lut(N, JET_SEGMENTS[c]) for c in ("red", "green", "blue")], 1)


def denormalize_roundtrip_table(mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
    """uint8 [3,256]: entry [c][v] = what the reference's overlay shows for a decoded byte v of channel c - datasets/transforms.normalize_img
    (numpy: float64 arithmetic, stored as float32) followed by utils/imutils.denormalize_img (torch CPU, float32, .type(torch.uint8)
    truncates).  Not the identity: 1 / 5 / 14 of the R / G / B values change."""
    import torch
    v = np.arange(256, dtype=np.uint8)
    imgarr = np.stack([v, v, v], -1)[None]                           # [1,256,3] HWC, like a decoded image
    proc = np.empty_like(imgarr, np.float32)
    for c in range(3):
        proc[..., c] = (imgarr[..., c] - mean[c]) / std[c]
    imgs = torch.from_numpy(proc).permute(2, 0, 1)[None]             # [1,3,1,256], the harness' input tensor
    out = torch.zeros_like(imgs)
    for c in range(3):
        out[:, c, :, :] = imgs[:, c, :, :] * std[c] + mean[c]
    return out.type(torch.uint8)[0, :, 0, :].numpy().copy()


def cam_overlay_tables(alpha, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
    """The two float64 tables excel_cam_overlay_ragged adds, [2,768]: [0] = alpha * (jet * 255) as [256][3]; [1] = (1 - alpha) * the
    round-trip image value as [3][256] - both terms of `alpha*cam_rgb + (1-alpha)*img` (:101-102) computed as numpy computes them, so
    the kernel's one add gives the reference's float64 sum."""
    lut = alpha * (jet_lut() * 255)
    img = (1 - alpha) * denormalize_roundtrip_table(mean, std).astype(np.float64)
    return np.ascontiguousarray(np.stack([lut.reshape(-1), img.reshape(-1)]))


def save_jpeg(path, rgb):
    """imageio.imsave(path, uint8 [H,W,3]) for a .jpg: Pillow at quality 75."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(rgb, np.uint8)).save(path, format="JPEG", quality=CAM_JPEG_QUALITY)
    return path


class CamOverlayWriter:
    """Device overlays -> JPEG files, off the launching thread.  submit() enqueues the D2H copy of a batch's overlay bytes into pinned
    memory on the current stream and records an event; a small thread pool waits for the event and encodes the files (Pillow releases
    the GIL), overlapping the next batches.  At most `max_pending` batches are in flight: submit() waits for the oldest beyond that
    (host back-pressure on the encoders, never a wait for the GPU in the launching thread).  close() waits for all and re-raises the
    first encoder error."""

    def __init__(self, threads=2, max_pending=None):
        import concurrent.futures as cf
        self.threads = max(1, int(threads))
        self._pool = cf.ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="cam_jpeg")
        self._pending = []
        self._max = max_pending or 2 * self.threads + 1
        self.files = 0

    @staticmethod
    def _encode(ev, host, items):
        ev.synchronize()
        buf = host.numpy()
        for path, off, H, W in items:
            save_jpeg(path, buf[off:off + 3 * H * W].reshape(H, W, 3))
        return len(items)

    def submit(self, dev_u8, items):
        """dev_u8: flat uint8 device tensor; items: [(path, byte offset, H, W)] of the overlays it holds."""
        import torch
        if not items:
            return
        host = torch.empty(dev_u8.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(dev_u8, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        while len(self._pending) >= self._max:
            self.files += self._pending.pop(0).result()
        self._pending.append(self._pool.submit(self._encode, ev, host, list(items)))

    def barrier(self):
        """Wait until every file submitted so far is on disk (re-raises the first encoder error); the writer stays usable."""
        while self._pending:
            self.files += self._pending.pop(0).result()

    def close(self):
        try:
            self.barrier()
        finally:
            self._pool.shutdown(wait=True)
        return self.files


# ------------------------------------------------------------------ label PNG files (tools/infer_lam.py:95, tools/training_free_attr.py:225)
class LabelPngWriter:
    """Device-encoded PNG files (ops.png_encode_labels_ragged) -> disk, off the launching thread.  submit() enqueues the D2H copy of a
    batch's arena and its (offset, size) table into one of `slots` pinned buffers on the current stream and records an event; once the
    event has completed the batch goes to a small thread pool that only does open / write / close.  Nothing on the host parses or patches
    the bytes: the sizes come from the table.
    The event discipline is DeviceFeeder's: every host-side look at an event (query, and the wait for the oldest one when the ring is
    full, which with 4 slots is several steps old) happens in the thread that recorded it; the pool threads never touch the GPU.  A
    pinned buffer is reused only after all its files are on disk; a writer's exception is raised by the next submit() or by close()."""

    def __init__(self, threads=2, slots=4):
        import concurrent.futures as cf
        self.threads = max(1, int(threads))
        self._pool = cf.ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="label_png")
        self._slots = [dict(bytes=None, table=None, futures=[]) for _ in range(max(2, int(slots)))]
        self._next = 0
        self._copying = []           # [(event, slot, paths)] in submission order: copies the GPU may not have finished
        self.files = 0
        self.bytes = 0

    @staticmethod
    def _write(buf, table, paths, lo, hi):
        n = 0
        for b in range(lo, hi):
            off, size = int(table[b, 0]), int(table[b, 1])
            with open(paths[b], "wb") as f:
                f.write(buf[off:off + size])
            n += size
        return hi - lo, n

    def _collect(self, slot):
        """Wait for the files of `slot` (re-raises a writer's exception)."""
        futures, slot["futures"] = slot["futures"], []
        err = None
        for fu in futures:
            try:
                k, n = fu.result()
                self.files += k
                self.bytes += n
            except BaseException as e:          # keep draining: the buffer must not be reused under a running writer
                err = err or e
        if err is not None:
            raise err

    def _dispatch(self, wait=False):
        """Hand the batches whose copy has completed to the pool (in order); wait=True: wait for the oldest one first."""
        while self._copying:
            ev, slot, paths = self._copying[0]
            if wait:
                ev.synchronize()
                wait = False
            elif not ev.query():
                return
            self._copying.pop(0)
            buf, table = memoryview(slot["bytes"].numpy()), slot["table"].numpy()
            B = len(paths)
            step = -(-B // self.threads)
            slot["futures"] = [self._pool.submit(self._write, buf, table, paths, lo, min(B, lo + step)) for lo in range(0, B, step)]

    def submit(self, dev_bytes, dev_table, paths):
        """dev_bytes, dev_table: what ops.png_encode_labels_ragged returned (queued on the current stream); paths: one file name per image."""
        import torch
        if len(paths) != int(dev_table.shape[0]):
            raise ValueError(f"{len(paths)} paths for {int(dev_table.shape[0])} images")
        self._dispatch()
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        while any(s is slot for _, s, _ in self._copying):      # the ring went round: its copy must land and its files be written
            self._dispatch(wait=True)
        self._collect(slot)
        if slot["bytes"] is None or slot["bytes"].numel() < dev_bytes.numel():
            slot["bytes"] = torch.empty(dev_bytes.numel(), dtype=torch.uint8, pin_memory=True)
        if slot["table"] is None or slot["table"].shape[0] < dev_table.shape[0]:
            slot["table"] = torch.empty((int(dev_table.shape[0]), 2), dtype=torch.int64, pin_memory=True)
        slot["bytes"][:dev_bytes.numel()].copy_(dev_bytes, non_blocking=True)
        slot["table"][:dev_table.shape[0]].copy_(dev_table, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._copying.append((ev, slot, [str(p) for p in paths]))

    def barrier(self):
        """Wait until every file submitted so far is on disk (re-raises the first writer's exception); the writer stays usable: a file
        submitted afterwards under the same name replaces the earlier one, never the other way round."""
        err = None
        while self._copying:
            self._dispatch(wait=True)
        for slot in self._slots:
            try:
                self._collect(slot)
            except BaseException as e:
                err = err or e
        if err is not None:
            raise err

    def close(self):
        """Wait for every file; -> the number of files written.  Re-raises the first writer's exception."""
        try:
            self.barrier()
        finally:
            self._pool.shutdown(wait=True)
        return self.files


# ------------------------------------------------------------------ device-encoded CAM overlay files (tools/infer_lam.py:104,111)
class CamJpegWriter(LabelPngWriter):
    """Device-encoded JPEG files (ops.jpeg_encode_rgb_ragged) -> disk: LabelPngWriter's ring of pinned buffers and its event discipline
    (every event wait in the launching thread, the pool threads only open / write / close).  A table entry of size -1 is a file that did
    not fit into the arena: when the batch is handed to the pool, the launching thread copies that one overlay's raw bytes from `rgb`
    and a pool thread encodes it with save_jpeg, which writes the same bytes.  `ratio` is the largest (file bytes / raw bytes) of a
    batch seen so far (None before the first batch has landed): what a caller sizes the next arena by."""

    def __init__(self, threads=2, slots=4):
        super().__init__(threads, slots)
        self.fallbacks = 0          # overlays encoded on the host (size -1 in the table)
        self.copied = 0             # bytes copied to the host
        self.ratio = None

    @staticmethod
    def _write(buf, table, paths, raw, lo, hi):
        n = 0
        for b in range(lo, hi):
            if b in raw:
                save_jpeg(paths[b], raw[b])
                continue
            off, size = int(table[b, 0]), int(table[b, 1])
            with open(paths[b], "wb") as f:
                f.write(buf[off:off + size])
            n += size
        return hi - lo, n

    def _hand_over(self, slot, paths, items, rgb):
        """The copy of `slot` has landed: its files -> the pool.  items: [(byte offset, H, W)] of the overlays in `rgb` (a flat uint8
        tensor, device or host)."""
        buf, table = memoryview(slot["bytes"].numpy()), slot["table"].numpy()
        B = len(paths)
        raw = {}
        for b, (off, H, W) in enumerate(items):
            if table[b, 1] < 0:
                raw[b] = rgb[int(off):int(off) + 3 * H * W].cpu().numpy().reshape(H, W, 3)
        self.fallbacks += len(raw)
        if not raw:
            r = float(table[:B, 1].sum()) / max(1, sum(3 * H * W for _, H, W in items))
            self.ratio = r if self.ratio is None else max(self.ratio, r)
        step = -(-B // self.threads)
        slot["futures"] = [self._pool.submit(self._write, buf, table, paths, raw, lo, min(B, lo + step)) for lo in range(0, B, step)]

    def _dispatch(self, wait=False):
        while self._copying:
            ev, slot, paths, items, rgb = self._copying[0]
            if wait:
                ev.synchronize()
                wait = False
            elif not ev.query():
                return
            self._copying.pop(0)
            self._hand_over(slot, paths, items, rgb)

    def submit(self, dev_bytes, dev_table, paths, items, rgb):
        """dev_bytes, dev_table: what ops.jpeg_encode_rgb_ragged returned (queued on the current stream); paths: one file name per image;
        items, rgb: what the encoder was given (rgb is kept alive until the batch has been handed to the pool)."""
        import torch
        if not (len(paths) == len(items) == int(dev_table.shape[0])):
            raise ValueError(f"{len(paths)} paths and {len(items)} items for {int(dev_table.shape[0])} images")
        self._dispatch()
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        while any(c[1] is slot for c in self._copying):
            self._dispatch(wait=True)
        self._collect(slot)
        if slot["bytes"] is None or slot["bytes"].numel() < dev_bytes.numel():
            slot["bytes"] = torch.empty(dev_bytes.numel(), dtype=torch.uint8, pin_memory=True)
        if slot["table"] is None or slot["table"].shape[0] < dev_table.shape[0]:
            slot["table"] = torch.empty((int(dev_table.shape[0]), 2), dtype=torch.int64, pin_memory=True)
        slot["bytes"][:dev_bytes.numel()].copy_(dev_bytes, non_blocking=True)
        slot["table"][:dev_table.shape[0]].copy_(dev_table, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.copied += int(dev_bytes.numel()) + 16 * int(dev_table.shape[0])
        self._copying.append((ev, slot, [str(p) for p in paths], [(int(o), int(h), int(w)) for o, h, w in items], rgb))
