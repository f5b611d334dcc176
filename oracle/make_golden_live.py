"""TEST INFRASTRUCTURE ONLY.  Stores what the UNMODIFIED reference returns for the seeded cases of five CPU tests, so
that those tests compare against it where the reference tree is absent:

    tests/golden/eval_map_reference.npz   mmdet/core/evaluation/mean_ap.py eval_map / tpfp_default on
                                          tests/test_eval_map.py's _case(seed) (reference_results)
    tests/golden/labelv2_reference.npz    mmdet/datasets/retinaface.py's reading of tests/test_datasets.py's
                                          random_label_file(seed) (reference_label_results)
    tests/golden/detect_rect_reference.npz  simple_test on tests/test_detect_oracle.py's rect_case(kind, h, w)
                                          (reference_rect_detections)
    tests/golden/wider_eval_live_reference.npz  wider_evaluation on tests/test_evaluation.py's LIVE_SEEDS
                                          (reference_aps)
    tests/golden/group_sampler_live_reference.npz  GroupSampler / DistributedGroupSampler orders on
                                          tests/test_samplers.py's live_cases() (reference_live_orders)

    python oracle/make_golden_live.py

The cases and the reference calls are the tests' own functions, run with live=True.
"""
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.join(HERE, '..', 'tests')
sys.path[:0] = [os.path.join(HERE, '..'), HERE, TESTS]
import test_datasets as TD  # noqa: E402
import test_detect_oracle as TDO  # noqa: E402
import test_eval_map as TE  # noqa: E402
import test_evaluation as TEV  # noqa: E402
import test_samplers as TS  # noqa: E402


def main():
    out = {f'{seed}/{k}': np.asarray(v) for seed in TE.SEEDS for k, v in TE.reference_results(seed, live=True).items()}
    np.savez_compressed(TE.STORED, **out)
    print('wrote', TE.STORED, len(out), 'arrays')

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for seed in range(12):
            _, infos, anns = TD.reference_label_results(Path(tmp) / 'l.txt', seed, live=True)
            out[f'{seed}/filename'] = np.array([n for n, _, _ in infos], dtype=str)
            out[f'{seed}/size'] = np.array([(w, h) for _, w, h in infos], dtype=np.int64).reshape(-1, 2)
            for i, a in enumerate(anns):
                out.update({f'{seed}/{i}/{k}': v for k, v in a.items()})
    np.savez_compressed(TD.STORED, **out)
    print('wrote', TD.STORED, len(out), 'arrays')

    out = {f'{kind}_{h}_{w}/{i}': d for kind, h, w in TDO.RECT_CASES
           for i, d in enumerate(TDO.reference_rect_detections(kind, h, w, live=True))}
    np.savez_compressed(TDO.RECT_STORED, **out)
    print('wrote', TDO.RECT_STORED, len(out), 'arrays')

    out = {str(seed): np.asarray(TEV.reference_aps(seed, live=True)) for seed in TEV.LIVE_SEEDS}
    np.savez_compressed(TEV.LIVE_STORED, **out)
    print('wrote', TEV.LIVE_STORED, len(out), 'arrays')

    out = {}
    for c, (ranks, group) in enumerate(TS.reference_live_orders(live=True)):
        out.update({f'{c}/rank{r}': o for r, o in enumerate(ranks)})
        out[f'{c}/group'] = group
    np.savez_compressed(TS.LIVE_STORED, **out)
    print('wrote', TS.LIVE_STORED, len(out), 'arrays')


if __name__ == '__main__':
    main()
