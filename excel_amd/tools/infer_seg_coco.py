"""COCO segmentation evaluation program: mirror of tools/infer_seg_coco.py, sharing the VOC program's loop (tools/infer_seg_voc.py).

What differs from VOC, all taken from the reference's two files:
  * defaults: --num_classes 81, --dataset_name ms_coco, --num_attri 224, --crf_post true, --list_folder datasets/coco;
  * data: datasets/coco.CocoSegDataset (JPEGImages/val, SegmentationClass/val, label names name[13:], grey JPEGs as 3 channels);
  * the scales are fused at (int(0.2 h), int(0.2 w)) (:63-64) with flip-averaging at every scale, scale 1.0 included (:73); an image
    whose 0.2x size is empty is an error.  The arg-max is taken at the label size through excel_seg_resize_argmax_ragged (:86-87): the
    81-class logits at full size never reach memory;
  * the CRF input is the fused logits resized from the small size to (H, W), then softmax (:144-145);
  * there is no test-set branch.
Like the VOC program, the CRF runs inline and no logits records are written.
    python -m excel_amd.tools.infer_seg_coco --model_path <run>/checkpoints/model_iter_N.pth --data_folder <MSCOCO2014> ...
"""
import logging

from . import infer_seg_voc
from .infer_seg_voc import SegVariant


class CocoVariant(SegVariant):
    name = "coco"
    fuse_factor = 0.2
    flip_first = True
    test_set = False

    @staticmethod
    def dataset(args, stage):
        from ..datasets import coco
        return coco.CocoSegDataset(root_dir=args.data_folder, name_list_dir=args.list_folder, split=args.infer_set, stage=stage,
                                   ignore_index=args.ignore_index)

    @staticmethod
    def class_list():
        from ..datasets import coco
        return coco.class_list


COCO = CocoVariant()


def get_parser():
    """The VOC program's flags with tools/infer_seg_coco.py's defaults (:24-44)."""
    p = infer_seg_voc.get_parser()
    p.set_defaults(num_classes=81, dataset_name="ms_coco", num_attri=224, crf_post=True, list_folder="datasets/coco")
    return p


def fuse_size(h, w):
    """(int(0.2 h), int(0.2 w)) (:63-64); ValueError when a side becomes 0."""
    return COCO.fuse_size(h, w)


def validate(args, model=None):
    return infer_seg_voc.validate(args, model=model, variant=COCO)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    validate(get_parser().parse_args())
