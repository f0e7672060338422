"""COCO decoder training: mirror of scripts/train_coco.py, sharing the VOC program's loop (scripts/train_voc.py: train, DecoderTrainer).

What differs from VOC, all taken from the reference's two files (`diff scripts/train_voc.py scripts/train_coco.py`):
  * defaults: --dataset_name ms_coco, the COCO attribute descriptors, --num_attri 224, --num_classes 81, --max_iters 100000,
    --warmup_iters 200, --eval_iters 100, --train_set train, --val_set val_part, --list_folder datasets/coco, --num_workers 4;
  * data: datasets/coco.CocoClsDataset (JPEGImages/train, grey JPEGs as 3 channels, no label map) and CocoSegDataset for validation;
    the training transform is the image-only one (ops.train_augment_image: random_crop(label=None) takes the first crop draw);
  * loop: caa_thre 0.88 (:193), the LVC switch (cure_attr_map on the head's features + seg_attn) at n_iter >= 30000 (:184-192), the
    affinity target is always the pseudo labels (:206, no switch to the seg arg-max);
  * checkpoints only from iteration 40000 on (:249), lowered with --save_ckpt_from;
  * validation with 81 classes and COCO's class names (:251);
  * --save_visual / tb_writer: five progress panels, no seg_gt (:229-242); seg_pred has the crop's size as in VOC (:199, :235).
Checkpoints are model_iter_N.pth with the head's keys, for `python -m excel_amd.tools.infer_seg_coco --model_path ...`.

  python -m excel_amd.scripts.train_coco --data_folder MSCOCO2014 --list_folder datasets/coco --model ViT-B-16.pt --bpe_path ...
  python -m torch.distributed.run --nproc-per-node R -m excel_amd.scripts.train_coco ...       (R ranks, gradients all-reduced)
"""
import logging

from .. import ops
from . import train_voc
from .train_voc import TrainVariant


class CocoVariant(TrainVariant):
    name = "coco"
    caa_thre = 0.88
    lvc_iter = 30000
    seg_aff_iter = None

    @staticmethod
    def datasets(args):
        from ..datasets import coco
        train = coco.CocoClsDataset(root_dir=args.data_folder, name_list_dir=args.list_folder, split=args.train_set, stage="train",
                                    aug=True, rescale_range=(0.5, 2.0), crop_size=args.crop_size, img_fliplr=True,
                                    ignore_index=args.ignore_index, num_classes=args.num_classes, seed=args.seed)
        val = coco.CocoSegDataset(root_dir=args.data_folder, name_list_dir=args.list_folder, split=args.val_set, stage="val",
                                  ignore_index=args.ignore_index)
        return train, val

    @staticmethod
    def augment(images, plan, labels, args):
        return ops.train_augment_image(images, plan, None, args.crop_size, aug_plan=plan.aug)[0]

    @staticmethod
    def augment_with_gt(images, plan, labels, args):
        """no label map in this data: the progress panels have no seg_gt (scripts/train_coco.py:234, :241)"""
        return CocoVariant.augment(images, plan, labels, args), None

    @staticmethod
    def class_list(args):
        from ..datasets import coco
        return coco.class_list if args.num_classes == 81 else None

    @staticmethod
    def first_ckpt_iter(args):
        return args.save_ckpt_from


COCO = CocoVariant()


def get_parser():
    """The VOC program's flags with scripts/train_coco.py's defaults (:29-82), plus --save_ckpt_from."""
    p = train_voc.get_parser()
    p.set_defaults(dataset_name="ms_coco", attr_json="./attributes_text/descriptors_ms_coco_gpt4.0_cluster_a_photo_of4.json",
                   num_attri=224, max_iters=100000, eval_iters=100, warmup_iters=200, data_folder="/data/Datasets/MSCOCO2014/",
                   list_folder="datasets/coco", num_classes=81, train_set="train", val_set="val_part", num_workers=4)
    p.add_argument("--save_ckpt_from", default=40000, type=int, help="first iteration whose validation writes a checkpoint (:249)")
    return p


def train(args, model=None, tb_writer=None):
    return train_voc.train(args, model=model, variant=COCO, tb_writer=tb_writer)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    train(get_parser().parse_args())
