"""The label stages behind the arg-max - snap, clean, fill, margin - described once, for the code that only carries them around:
tools/infer_lam.py, tools/eval_labels.py, utils/image_scores.py and pipeline.py loop over this table.  What a stage computes lives in
its own module (utils/superpixels.py, components.py, label_fill.py, margin.py) and in the pipeline's _snap / _clean / _fill / _margin;
here is only what the call sites differ in, and the order of the stages in every place where an order can be seen.  Host only: numpy.

A stage's `name` is its score set in image_scores.SETS, its key in --json_out and in the programs' reports, and the stem of what a
pipeline keeps for it: hist_<name>, last_<name>_labels and, with a row set, last_<name>_counts.
"""
from collections import namedtuple

import numpy as np

from . import components, label_fill, margin, superpixels

# the per-image rows of a stage ([N,3] integers): `key` in ImageScoreLog's records, the merged table and the npz; the three CSV
# heads; cells(row, fmt) -> the three CSV cells (fmt: image_scores' float format)
RowSet = namedtuple("RowSet", "key heads cells")
_ints = lambda row, fmt: [int(v) for v in row]

# flag     the leading flag, for messages
# kwarg    the pipelines' keyword; its value is the dict of the resolved `keys`, or for a bare string the one resolved value
# resolve  (args, program="infer_lam", ragged=None) -> the resolved flags as a dict (with label_dir), or None: the stage is off
# noun     of the log line "<noun> label maps -> <label_dir>"
# params   resolved -> the bracket of the score table's title
# stats    [N,3] rows -> the stage's totals (snap: also the pixel total);  summary(stats, coverage) -> the log's summary, or None
# json     (resolved, stats, score, coverage) -> the stage's block of --json_out
Stage = namedtuple("Stage", "name flag kwarg keys resolve rows noun params stats summary json")


def _resolver(module):
    return lambda args, program="infer_lam", ragged=None: module.resolve(args, program=program)


def _resolve_margin(args, program="infer_lam", ragged=None):
    """margin.resolve also answers for --margin_sweep, and refuses a run without ragged batches itself (it names the flag given)."""
    return margin.resolve(args, ragged=ragged)[1]


def _margin_summary(stats, cover):
    return None if cover is None else f"margin coverage (kept pixels over labelled pixels): {cover * 100:.3f} %"


STAGES = {s.name: s for s in (
    Stage("snap", "--snap_superpixels", "snap", ("step", "compactness", "iters", "min_share"), _resolver(superpixels),
          RowSet("snaps", ("superpixels", "snapped", "pixels_changed"), _ints), "snapped",
          lambda r: f"--snap_superpixels {r['step']}, compactness {r['compactness']}, {r['iters']} iterations, min share {r['min_share']:g}",
          superpixels.snap_stats, superpixels.format_snap_summary, superpixels.snap_json),
    Stage("clean", "--clean_min_region", "clean", ("min_region", "connectivity"), _resolver(components),
          RowSet("regions", ("regions", "regions_removed", "pixels_removed"), _ints), "cleaned",
          lambda r: f"--clean_min_region {r['min_region']:g}, connectivity {r['connectivity']}",
          components.region_stats, components.format_clean_summary,
          lambda r, stats, score, cover: components.clean_json(r["min_region"], r["connectivity"], stats, score, cover)),
    Stage("fill", "--fill_ignore", "fill", ("radius",), _resolver(label_fill),
          RowSet("fills", ("holes", "filled", "max_fill_dist"), lambda row, fmt: [int(row[0]), int(row[1]), fmt(np.sqrt(float(row[2])))]),
          "filled", lambda r: f"--fill_ignore {'inf' if r['radius'] is None else r['radius']}",
          label_fill.fill_stats, label_fill.format_fill_summary,
          lambda r, stats, score, cover: label_fill.fill_json(r["radius"], stats, score, cover)),
    Stage("margin", "--margin_min", "margin_min", "min", _resolve_margin, None, "margin",
          lambda r: f"--margin_min {r['min']:g}", None, _margin_summary,
          lambda r, stats, score, cover: margin.margin_min_json(r["min"], score, cover)))}

# The orders, one per place where an order can be seen.  They differ for historical reasons and are part of what the programs write.
CHAIN_ORDER = ("snap", "clean", "fill")                     # what feeds what in a step: run_batch_ragged, eval_labels' batches
ROW_SET_ORDER = ("clean", "fill", "snap")                   # the last columns of --per_image_scores' CSV, the arrays of its npz
INFER_LAM_ORDER = ("clean", "fill", "snap", "margin")       # infer_lam: resolving and refusing, gathering over the ranks, the log
INFER_LAM_JSON_ORDER = ("margin", "clean", "fill", "snap")  # infer_lam: the blocks of the --json_out record
EVAL_LABELS_ORDER = ("snap", "clean", "fill")               # eval_labels: gathering over the ranks, the log
ROW_SETS = tuple(STAGES[n].rows for n in ROW_SET_ORDER)


def pipeline_value(stage, resolved):
    """What the pipelines take as `<stage.kwarg>=` and keep under that name, from the stage's resolved flags."""
    return resolved[stage.keys] if isinstance(stage.keys, str) else {k: resolved[k] for k in stage.keys}


def title(stage, resolved, of=None):
    """The line above the stage's score table; `of`: what was scored, where the program names it (eval_labels' --pred_dir)."""
    return f"{stage.name}_label_score{'' if of is None else ' of ' + str(of)} ({stage.params(resolved)}):"
