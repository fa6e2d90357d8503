"""motion324_amd.video_metrics with stub scorers: the reference's file name, line order and rule, for any subset of the metrics."""
import os

import numpy as np
import pytest

from motion324_amd import video_metrics as VM
from motion324_amd.lib import M324Error


def make_pairs(tmp_path, n=2):
    gts, results = [], []
    for i in range(n):
        g, r = tmp_path / f"gt{i}.npy", tmp_path / "runs" / f"clip{i}.npy"
        r.parent.mkdir(exist_ok=True)
        for p in (g, r):
            np.save(p, np.zeros((1,), np.uint8))
        gts.append(str(g))
        results.append(str(r))
    return gts, results


def test_all_four_lines_in_the_reference_order(tmp_path):
    gts, results = make_pairs(tmp_path)
    seen = []
    scorers = {"CLIP Loss": lambda a, b: 0.75, "DreamSim": lambda a, b: 0.125, "FVD": lambda a, b: 321.5, "LPIPS": lambda a, b: 0.25}
    done = VM.evaluate_pairs(gts, results, scorers, str(tmp_path / "out"), load=lambda p: seen.append(p) or p, log=lambda s: None)
    assert [os.path.basename(f) for f, _ in done] == ["clip0.txt", "clip1.txt"] and seen == [gts[0], results[0], gts[1], results[1]]
    text = open(tmp_path / "out" / "clip1.txt").read()
    assert text == (f"GT Source: {gts[1]}\nResult Source: {results[1]}\nFVD: 321.5\nLPIPS: 0.25\nDreamSim: 0.125\nCLIP Loss: 0.75\n"
                    + "-" * 50 + "\n")
    assert list(done[0][1]) == list(VM.ORDER)


def test_a_subset_writes_its_lines_only_and_defaults_to_the_results_directory(tmp_path):
    gts, results = make_pairs(tmp_path, 1)
    lines = []
    done = VM.evaluate_pairs(gts, results, {"DreamSim": lambda a, b: 0.5, "FVD": lambda a, b: 2.0}, load=lambda p: p, log=lines.append)
    assert done[0][0] == str(tmp_path / "runs" / "clip0.txt")
    assert open(done[0][0]).read().splitlines() == [f"GT Source: {gts[0]}", f"Result Source: {results[0]}", "FVD: 2.0", "DreamSim: 0.5", "-" * 50]
    assert lines[-1] == "Summary: processed 1/1 pairs; Average FVD: 2.000000; Average DreamSim: 0.500000"


def test_directories_keep_their_name_and_missing_pairs_are_skipped(tmp_path):
    frames = tmp_path / "result_frames"
    frames.mkdir()
    assert VM.result_file(str(frames) + "/", "out") == os.path.join("out", "result_frames.txt")
    lines = []
    done = VM.evaluate_pairs([str(tmp_path / "nothing.npy")], [str(frames)], {"LPIPS": lambda a, b: 1.0}, load=lambda p: p, log=lines.append)
    assert done == [] and lines[0].startswith("Warning:") and lines[-1] == "Summary: processed 0/1 pairs"


def test_refusals():
    with pytest.raises(M324Error, match="non-empty subset"):
        VM.evaluate_pairs([], [], {})
    with pytest.raises(M324Error, match="non-empty subset"):
        VM.evaluate_pairs([], [], {"PSNR": lambda a, b: 0.0})
    with pytest.raises(M324Error, match="matched by position"):
        VM.evaluate_pairs(["a", "b"], ["c"], {"FVD": lambda a, b: 0.0})
    with pytest.raises(M324Error, match="unknown metric"):
        VM.format_result("a", "b", {"SSIM": 1.0})
    with pytest.raises(M324Error, match="all three"):
        VM.main(["--gt_paths", "a", "--result_paths", "b", "--dino", "x"])
    with pytest.raises(M324Error, match="at least one metric"):
        VM.main(["--gt_paths", "a", "--result_paths", "b"])
