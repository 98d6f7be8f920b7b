"""Pre-compute the ``heuristic_intent`` column of every log — the reference's
preprocess_intent_labels.py:16-139 with the labelling on the GPU.

Same arguments (``--data_root``, ``--splits``, ``--force``), same output file next to each
log's annotations (``annotations_with_intent.feather``: every input column untouched plus
``heuristic_intent``) and the same "processed" / "skipped" / "failed" results. The reference
calls its heuristic once per annotation row (:41-57), each call filtering and sorting the
whole table; here a log is one launch (heuristic_labeling.label_annotations).

Map context is not implemented: the labels are those of the reference's map-free branch
(``av2`` not importable), whether or not a log has a map directory.
"""
from __future__ import annotations

import argparse
import time
from pathlib import Path

import pandas as pd

from dataset import ScenarioValidator
from heuristic_labeling import label_annotations

OUTPUT_ANNOTATION_FILENAME = "annotations_with_intent.feather"


def preprocess_scenario(scenario_info, force_recompute: bool = False, device=None) -> str:
    """preprocess_intent_labels.py:16-63 for one scenario -> "processed" | "skipped" | "failed"."""
    log_dir = Path(scenario_info.log_dir)
    log_id = log_dir.name
    output_path = log_dir / OUTPUT_ANNOTATION_FILENAME
    if not force_recompute and output_path.exists():
        return "skipped"
    try:
        annotations_df = pd.read_feather(Path(scenario_info.annotations_path))
        annotations_df['heuristic_intent'] = label_annotations(annotations_df, device=device)
        annotations_df.to_feather(output_path)
        return "processed"
    except Exception as e:  # noqa: BLE001  (the reference's behaviour, :61-63)
        print(f"  ERROR processing scenario {log_id}: {e}")
        return "failed"


def main(data_root_dir: str, splits: list[str] | None = None, force_recompute: bool = False, device=None) -> dict:
    """preprocess_intent_labels.py:65-120. Returns the totals it prints
    ({"processed", "skipped", "failed"}; the reference returns None)."""
    if splits is None:
        splits = ["train", "val"]
    print("Starting intention label pre-computation.")
    print(f"Output file name per log: {OUTPUT_ANNOTATION_FILENAME}")
    print(f"Force recompute: {force_recompute}")
    t0 = time.time()
    total = {"processed": 0, "skipped": 0, "failed": 0}
    for split_name in splits:
        print(f"\nProcessing split: {split_name}")
        split_dir = Path(data_root_dir) / split_name
        if not split_dir.is_dir():
            print(f"  Directory for split '{split_name}' not found at: {split_dir}. Skipping.")
            continue
        valid_scenarios = ScenarioValidator(str(split_dir), skip_known_corrupted=False).find_valid_scenarios()
        if not valid_scenarios:
            print(f"  No valid scenarios found in {split_dir}.")
            continue
        print(f"  Found {len(valid_scenarios)} scenarios in {split_name} split.")
        split = {"processed": 0, "skipped": 0, "failed": 0}
        for scenario_info in valid_scenarios:
            split[preprocess_scenario(scenario_info, force_recompute, device)] += 1
        print(f"  Finished {split_name} split: Processed={split['processed']}, Skipped={split['skipped']}, "
              f"Failed={split['failed']}")
        for k, v in split.items():
            total[k] += v
    print("\nPre-computation finished for all specified splits.")
    print(f"  Total time taken: {(time.time() - t0) / 60:.2f} minutes")
    print(f"  Total Scenarios Processed Successfully: {total['processed']}")
    print(f"  Total Scenarios Skipped (Already Done): {total['skipped']}")
    print(f"  Total Scenarios Failed: {total['failed']}")
    return total


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Pre-compute vehicle intention labels for Argoverse 2 dataset.")
    parser.add_argument("--data_root", type=str, required=True,
                        help="Root directory of the Argoverse 2 sensor dataset (the directory containing the "
                             "'train', 'val', 'test' splits).")
    parser.add_argument("--splits", nargs='+', default=["train", "val"],
                        help="List of dataset splits to process (e.g., train val). Default is 'train' and 'val'.")
    parser.add_argument("--force", action="store_true",
                        help="Force re-computation even if output files already exist.")
    args = parser.parse_args()
    main(data_root_dir=args.data_root, splits=args.splits, force_recompute=args.force)
