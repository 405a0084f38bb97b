"""The text aligner's host side (no GPU): the shim's state_dict against the reference's key list, the float64 dynamic programme of
tests/aligner64.py against a brute-force enumeration of every valid path, its post-processing on a crafted path, and the shim's ValueErrors."""
import json
import os

import numpy as np
import pytest

import aligner64 as A

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_state_dict_keys_and_shapes_equal_the_reference():
    torch = pytest.importorskip("torch")  # noqa: F841
    from stylish_tts_amd import modules

    g = np.load(os.path.join(GOLD, "aligner_misc.npz"))
    keys, shapes = json.loads(str(g["keys"])), json.loads(str(g["shapes"]))
    sd = modules.TextAligner(80, 178).state_dict()
    assert list(sd.keys()) == keys
    assert [list(v.shape) for v in sd.values()] == shapes
    for want in ("encoder.layers.0.0.weight", "encoder.layers.2.2.running_var", "encoder.layers.1.2.num_batches_tracked", "encoder.layers.3.ffn.12.bias",
                 "encoder_output_layer.weight"):
        assert want in sd
    assert tuple(sd["encoder_output_layer.weight"].shape) == (179, 640) and tuple(sd["encoder.layers.0.0.weight"].shape) == (640, 80, 5)


def test_synthetic_batchnorm_statistics_are_not_trivial():
    pytest.importorskip("torch")
    from stylish_tts_amd import aligner, modules

    sd = modules.TextAligner().load_synthetic(0).state_dict()
    for i in range(3):
        m, v = sd[f"encoder.layers.{i}.2.running_mean"].numpy(), sd[f"encoder.layers.{i}.2.running_var"].numpy()
        assert np.abs(m).max() > 0.05 and v.min() > 0.4 and v.std() > 0.1
        sc, sh = aligner.fold_batchnorm(m, v)
        x = np.linspace(-1, 2, 640)
        assert np.allclose(x * sc + sh, (x - m.astype(np.float64)) / np.sqrt(v.astype(np.float64) + 1e-5), atol=1e-6)


def _lp(name, T, V):
    from stylish_tts_amd import synth

    return -8.0 * synth.uniform("aligner.cpu." + name, (T, V)).astype(np.float64)


@pytest.mark.parametrize("targets", [[1], [0, 1], [2, 2], [0, 1, 0], [1, 1, 2], [2, 0, 0], [1, 1, 1]])
def test_float64_dp_equals_brute_force(targets):
    V, blank = 4, 3
    need = A.min_frames(targets)
    for T in range(need, 9):
        lp = _lp(f"{targets}.{T}", T, V)
        path, best = A.viterbi(lp, targets, blank)
        assert best == pytest.approx(A.brute_force(lp, targets, blank), abs=1e-12), (targets, T)
        A.path_states(path, targets, blank)
        assert A.path_score(lp, path) == pytest.approx(best, abs=1e-12)
        d = A.durations(path, len(targets), blank)
        assert d.sum() == T and d.min() >= 1
        p1, b1 = A.viterbi(lp, targets, blank, leading_blank=False)
        assert p1[0] == targets[0] and b1 <= best + 1e-12
    with pytest.raises(ValueError):
        A.viterbi(_lp("short", need - 1, V) if need > 1 else np.zeros((0, V)), targets, blank)


def test_path_checker_names_every_broken_rule():
    tg, b = [1, 1, 2], 3
    A.path_states([1, 3, 1, 2], tg, b)
    A.path_states([3, 1, 3, 1, 2, 3], tg, b)
    for bad in ([2, 3, 1, 2], [1, 1, 2, 2], [1, 3, 2, 2], [1, 3, 1, 3], [1, 3, 1, 2, 1], []):
        with pytest.raises(ValueError):
            A.path_states(bad, tg, b)


def test_durations_and_boundaries_of_a_crafted_path():
    tg, b = [1, 1, 2], 3
    path = [b, b, 1, 1, b, 1, 2, 2, b]  # two leading blanks: they count to token 0 (the stated deviation from the reference's loop)
    d = A.durations(path, 3, b)
    assert d.tolist() == [5, 1, 3]
    lp = _lp("crafted", len(path), 4)
    left, right = A.boundaries(lp, tg, d)
    assert left[2] == 0 and right[2] == 0
    # the boundary between token 0 and token 1: equal tokens, so all three products are the same
    assert left[0] == pytest.approx(1 / 3) and right[0] == pytest.approx(1 / 3)
    i = 6
    want = np.exp(lp[i - 1, 1] + lp[i, 1]) / (np.exp(lp[i - 1, 1] + lp[i, 1]) + np.exp(lp[i - 1, 1] + lp[i, 2]) + np.exp(lp[i - 1, 2] + lp[i, 2]))
    assert left[1] == pytest.approx(want, rel=1e-14)


def test_unsupported_specs_and_infeasible_alignments_raise_value_error():
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import aligner, modules

    with pytest.raises(ValueError, match="blstm"):
        modules.TextAligner(80, 178, tdnn_blstm_spec=[("tdnn", 5, 1, 1), ("blstm",), ("ffn", 5)])
    for spec in ([("tdnn", 3, 2, 1), ("ffn", 5)], [("tdnn", 3, 1, 2), ("ffn", 5)], [("tdnn", 4, 1, 1), ("ffn", 5)], [("ffn", 5)], [("tdnn", 3, 1, 1)],
                 [("ffn", 2), ("tdnn", 3, 1, 1)], [("lstm",)]):
        with pytest.raises(ValueError):
            aligner.dims(80, 178, 640, spec)
    assert aligner.dims()["tdnn_kernel"] == [5, 3, 3] and aligner.dims()["classes"] == 179
    assert aligner.min_frames([4, 4, 5, 5, 5]) == 8
    aligner.check_alignable(8, [4, 4, 5, 5, 5])
    with pytest.raises(ValueError, match="frames"):
        aligner.check_alignable(7, [4, 4, 5, 5, 5])
    with pytest.raises(ValueError, match="tokens"):
        aligner.check_alignable(2000, list(range(511)))
    # the shim refuses an infeasible pair before it touches the engine
    m = modules.TextAligner()
    with pytest.raises(ValueError, match="frames"):
        m.align(torch.zeros(1, 3, 80), [3], torch.tensor([[7, 7, 8]]), [3])
    with pytest.raises(ValueError):
        m.align(torch.zeros(1, 3, 80), [3], torch.tensor([[7, 200]]), [2])


def test_checkpoint_reader_takes_the_text_aligner(tmp_path):
    torch = pytest.importorskip("torch")
    from stylish_tts_amd import checkpoint, modules

    src = modules.TextAligner().load_synthetic(1)
    sd = {"module." + k: v for k, v in src.state_dict().items()}  # a DistributedDataParallel-wrapped save
    torch.save(sd, tmp_path / "pytorch_model.bin")  # model index 0 of build_model
    got = checkpoint.load_accelerate_checkpoint(str(tmp_path), checkpoint.ALIGNER_MODULES)
    dst = modules.TextAligner()
    checkpoint.load_into({"text_aligner": dst}, got)
    assert all(torch.equal(a, b) for a, b in zip(src.state_dict().values(), dst.state_dict().values()))
    assert float(dst.state_dict()["encoder.layers.1.2.running_var"].min()) > 0.4
