"""Training-progress images: mirror of the parts of utils/tbutils.py the training programs use (scripts/train_voc.py:233-246).

  make_grid_image / make_grid_label   utils/tbutils.py:36-61, :88-93 over ops.train_panels (trainviz.hip): the same CHW uint8 grids
  TAGS / render_panels / log_panels   the six add_image calls of the training loop, all panels of a batch in one launch
  PanelWriter                         the grids as PNG files (<visual_dir>/iter_<N>/<panel>.png), written by one thread

make_grid_image_bkg, make_grid_attention and make_grid_attr_map are not used by the reference's programs and are not mirrored.
Neither tensorboard nor torchvision is needed: an object with add_image(tag, chw_uint8, global_step=) can be handed to
scripts.train_voc.train(tb_writer=...).
"""
import os
import queue
import threading

from .. import ops

TAGS = tuple("visual/" + n for n in ops.TRAIN_PANELS)       # the reference's tags, in the order of its add_image calls


def make_grid_image(img, cam, nrow=2, cls_label=None, mask=None):
    """img f32 [B,3,S,S] normalised, cam = attr_maps_raw [B,P,F], cls_label [B,F] -> (grid_img, grid_cam) uint8 [3,Hg,Wg] on the device."""
    if mask is not None:
        raise NotImplementedError("make_grid_image(mask=...) is not used by the training programs and not built")
    if cls_label is None:
        raise ValueError("make_grid_image needs cls_label (utils/tbutils.py:39)")
    p = ops.train_panels(inputs=img, attr_maps_raw=cam, cls_label=cls_label, nrow=nrow, panels=("img1", "cam1"))
    return p["img1"].permute(2, 0, 1), p["cam1"].permute(2, 0, 1)


def make_grid_label(label, nrow=2):
    """label [B,H,H] (any integer dtype, values 0..255) -> uint8 [3,Hg,Wg] on the device, coloured with the VOC palette."""
    import torch
    p = ops.train_panels(pseu_aff=label.to(torch.uint8), nrow=nrow, panels=("pseu_aff",))
    return p["pseu_aff"].permute(2, 0, 1)


def render_panels(inputs, cls_labels, step_out, seg_gt=None, nrow=2):
    """The panels of one training iteration from DecoderTrainer.train_step(want_visual=True)'s dict (seg_gt None: the COCO program's
    five) -> ops.TrainPanels."""
    return ops.train_panels(inputs=inputs, attr_maps_raw=step_out["attr_maps_raw"], cls_label=cls_labels, pseu_aff=step_out["aff_pseudos"],
                            pseu_mid=step_out["pseu_mid"], seg_gt=seg_gt, seg_pred=step_out["seg_pred"], nrow=nrow)


def log_panels(tb_writer, panels, global_step):
    """The add_image calls of :240-246 in the reference's order: every panel present in `panels` (name -> uint8 [Hg,Wg,3]) as CHW."""
    for name, tag in zip(ops.TRAIN_PANELS, TAGS):
        if name in panels:
            tb_writer.add_image(tag, panels[name].permute(2, 0, 1), global_step=global_step)


class PanelWriter:
    """Host panels -> PNG files off the training thread: ONE writer thread takes (directory, {name: uint8 [H,W,3]}) jobs in order.
    close() joins it and re-raises the first write error."""

    def __init__(self):
        self._q = queue.Queue()
        self._err = None
        self.dirs = []
        self._t = threading.Thread(target=self._run, name="panel_png", daemon=True)
        self._t.start()

    def _run(self):
        from PIL import Image
        while True:
            job = self._q.get()
            if job is None:
                return
            if self._err is not None:
                continue                      # keep draining so close() never waits on a full queue
            try:
                d, panels = job
                os.makedirs(d, exist_ok=True)
                for name, rgb in panels.items():
                    Image.fromarray(rgb).save(os.path.join(d, name + ".png"), format="PNG")
            except BaseException as e:
                self._err = e

    def submit(self, directory, panels):
        self.dirs.append(directory)
        self._q.put((directory, panels))

    def close(self):
        self._q.put(None)
        self._t.join()
        if self._err is not None:
            raise self._err
        return self.dirs
