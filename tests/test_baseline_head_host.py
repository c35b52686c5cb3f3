"""CPU: the organiser-baseline prediction path around the model call -- the float64 statement of pooling + head against what the
reference's own modules gave (tests/golden/baseline_head.npz, tools/make_baseline_head_golden.py), the loader's refusals, the
driver's file selection / cut / scaling / CSV rules around a stub predictor, and the new launchers' argument validation."""
import csv
import ctypes
import json
import os
import pickle
import wave as _wave

import numpy as np
import pytest
import torch

import asp_ref as R
from interspeech_ser_amd import baseline as BL

WAV_MEAN, WAV_STD = np.float64(-8.0614e-05), np.float64(0.0886208)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "baseline_head.npz"))
    pool = {k[len("pool."):]: z[k] for k in z.files if k.startswith("pool.")}
    ser = {n: {k[len(f"ser{n}."):]: z[k] for k in z.files if k.startswith(f"ser{n}.")} for n in (8, 3)}
    return z, pool, ser


def test_float64_statement_matches_the_reference_modules(fixture):
    """2e-5 relative to max(1, max|ref|), the bound of tests/test_oracle_golden.py.  The reference's fp32 arithmetic sits 4.5e-6 / 8e-7 /
    1.8e-6 (pooled / 8 logits / 3 logits) from the float64 statement on zero-mean inputs of these shapes; inputs with a column mean of 30
    and std 0.1 would put it at 6.2e-5 through the fp32 cancellation in m2 - mu^2, so the fixture holds none."""
    z, pool, ser = fixture
    offs = [int(v) for v in z["frame_offs"]]
    assert [b - a for a, b in zip(offs, offs[1:])] == [1, 2, 70, 333] and z["x"].shape[1] == 64
    pooled = R.asp_pool(z["x"], offs, pool)
    e = R.rel_err(z["pooled"], pooled)
    print(f"pooled rows: {e:.2e} (bound 2e-5)")
    assert e < 2e-5
    assert np.array_equal(pooled[0, :64], z["x"][0].astype(np.float64))                     # one frame: mu = x
    assert np.allclose(pooled[0, 64:], np.sqrt(np.float64(np.float32(1e-5))), rtol=0, atol=0)
    for n in (8, 3):
        assert ser[n]["fc.0.0.weight"].shape == (96, 128)
        e = R.rel_err(z[f"logits{n}"], R.mlp_head(pooled, ser[n]))
        print(f"logits n_out={n}: {e:.2e} (bound 2e-5)")
        assert e < 2e-5


def test_key_lists_equal_the_loaders_expectation(fixture):
    z, _, _ = fixture
    assert tuple(z["pool_keys"]) == BL.POOL_KEYS
    assert tuple(z["ser_keys"]) == BL.SER_KEYS


def _save_model_dir(path, D=64, H=96, n_out=8, extra=None):
    pool, ser = BL.synthetic_head_state_dicts(D, H, n_out, seed=3)
    ser.update(extra or {})
    os.makedirs(path, exist_ok=True)
    torch.save(pool, os.path.join(path, "final_pool.pt"))
    torch.save(ser, os.path.join(path, "final_ser.pt"))
    with open(os.path.join(path, "train_norm_stat.pkl"), "wb") as f:
        pickle.dump((WAV_MEAN, WAV_STD), f)
    return str(path)


def test_loader_reads_a_model_directory(tmp_path):
    pool, ser, mean, std = BL.load_baseline_head(_save_model_dir(tmp_path / "m"), 64, 96, 8)
    assert tuple(pool) == BL.POOL_KEYS and tuple(ser) == BL.SER_KEYS
    assert mean == WAV_MEAN and std == WAV_STD


def test_loader_refuses_a_second_hidden_layer(tmp_path):
    d = _save_model_dir(tmp_path / "m", extra={"fc.1.0.weight": torch.zeros(96, 96), "fc.1.0.bias": torch.zeros(96)})
    with pytest.raises(BL.HeadError, match="more than one hidden layer"):
        BL.load_baseline_head(d, 64, 96, 8)


def test_loader_refuses_a_wrong_head_dim(tmp_path):
    d = _save_model_dir(tmp_path / "m")
    with pytest.raises(BL.HeadError, match="--head_dim 1024"):
        BL.load_baseline_head(d, 64, 1024, 8)
    with pytest.raises(BL.HeadError, match="3 outputs"):
        BL.load_baseline_head(d, 64, 96, 3)


def test_loader_refuses_an_unknown_pooling_type(tmp_path):
    d = _save_model_dir(tmp_path / "m")
    with pytest.raises(BL.HeadError, match="MeanPooling"):
        BL.load_baseline_head(d, 64, 96, 8, pooling_type="MeanPooling")


# ------------------------------------------------------------------------------- driver around a stub predictor
def _write_wav(path, samples_i16):
    with _wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(16000)
        wf.writeframes(np.asarray(samples_i16, dtype="<i2").tobytes())


class _Stub:
    """Stands in for BaselinePredictor: same ``prepare``, logits looked up by the length of the prepared waveform."""
    SLOTS = 2

    def __init__(self, table, n_out):
        self.table, self.n_out, self.seen = table, n_out, {}

    def prepare(self, wav):
        return np.ascontiguousarray(BL.scale_wave(BL.cut_wave(wav), WAV_MEAN, WAV_STD))

    def extract(self, waves, layer_index=None, rates=None):
        for w in waves:
            self.seen[len(w)] = w
        return np.stack([np.asarray(self.table[len(w)], dtype=np.float32) for w in waves])

    def submit(self, waves, layer_index=None, slot=0, rates=None):
        return dict(out=self.extract(waves))

    def collect(self, ticket):
        return ticket["out"]


LENGTHS = {"b_test3_2.wav": 5000, "a_test3_1.wav": 4000, "long_test3.wav": 13 * 16000, "c_dev_3.wav": 6000, "z_test3_9.wav": 7000}


@pytest.fixture()
def corpus(tmp_path, built_library):
    wav_dir = tmp_path / "Audios"
    wav_dir.mkdir()
    rng = np.random.default_rng(5)
    pcm = {}
    for name, n in LENGTHS.items():
        pcm[name] = rng.integers(-20000, 20000, size=n).astype(np.int16)
        _write_wav(wav_dir / name, pcm[name])
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps({"wav_dir": str(wav_dir), "label_path": str(tmp_path / "labels_that_do_not_exist.csv")}))
    model = tmp_path / "model"
    model.mkdir()
    return dict(wav_dir=wav_dir, cfg=str(cfg), model=str(model), pcm=pcm)


def _run(kind, corpus, table, extra=(), n_out=None):
    stub = _Stub(table, n_out or BL.N_OUT[kind])
    fn = BL.run_eval_cat if kind == "cat" else BL.run_eval_dim
    rc = fn(["--model_path", corpus["model"], "--config_path", corpus["cfg"], "--batch_size", "2", *extra],
            predictor_factory=lambda args, k, device: stub)
    assert rc == 0
    return stub


def _read_csv(corpus, subset="test3"):
    with open(os.path.join(corpus["model"], "results", subset + ".csv"), newline="") as f:
        return list(csv.reader(f))


def _onehot(i, n=8):
    v = np.full(n, -1.0, dtype=np.float32)
    v[i] = 2.0
    return v


CAT_TABLE = {4000: _onehot(2), 5000: _onehot(7), 192000: _onehot(0), 7000: _onehot(5), 6000: _onehot(1)}


def test_driver_takes_the_test3_files_only_sorted_by_name(corpus, capsys):
    stub = _run("cat", corpus, CAT_TABLE)
    rows = _read_csv(corpus)
    assert rows[0] == ["FileName", "EmoClass"]
    assert [r[0] for r in rows[1:]] == ["a_test3_1.wav", "b_test3_2.wav", "long_test3.wav", "z_test3_9.wav"]
    assert 6000 not in stub.seen                                  # the file without the tag never reached the model
    assert "4 rows written" in capsys.readouterr().out


def test_driver_subset_flag_selects_files_and_names_the_csv(corpus):
    _run("cat", corpus, CAT_TABLE, extra=["--subset", "dev"])
    rows = _read_csv(corpus, "dev")
    assert rows[1:] == [["c_dev_3.wav", "S"]]


def test_driver_cuts_to_192000_samples(corpus):
    stub = _run("cat", corpus, CAT_TABLE)
    assert 13 * 16000 not in stub.seen and len(stub.seen[192000]) == 192000


def test_driver_scaling_is_the_reference_expression_bit_for_bit(corpus):
    stub = _run("cat", corpus, CAT_TABLE)
    for name in ("a_test3_1.wav", "long_test3.wav"):
        wav = (corpus["pcm"][name].astype(np.float32) / 32768.0)[:192000]          # what soundfile yields for 16-bit PCM
        want = ((wav - WAV_MEAN) / (WAV_STD + 0.000001)).astype(np.float32)
        got = stub.seen[len(want)]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_cat_csv_letters(corpus):
    _run("cat", corpus, CAT_TABLE)
    rows = dict(_read_csv(corpus)[1:])
    assert rows == {"a_test3_1.wav": "H", "b_test3_2.wav": "N", "long_test3.wav": "A", "z_test3_9.wav": "D"}
    assert BL.CAT_LETTERS == ("A", "S", "H", "U", "F", "D", "C", "N")


def test_dim_csv_clamps_and_swaps_valence_and_dominance(corpus):
    table = {4000: [0.5, 0.25, 0.75], 5000: [-0.3, 1.2, 0.0], 192000: [1.0, 0.0, 2.0], 7000: [0.1, 0.2, 0.3], 6000: [0, 0, 0]}
    _run("dim", corpus, table)
    rows = _read_csv(corpus)
    assert rows[0] == ["FileName", "EmoAct", "EmoVal", "EmoDom"]
    got = {r[0]: [float(v) for v in r[1:]] for r in rows[1:]}
    f = lambda v: min(max(1, float(np.float32(v)) * 6 + 1), 7)                      # noqa: E731
    assert got["a_test3_1.wav"] == [f(0.5), f(0.75), f(0.25)]                       # EmoVal = pred[2], EmoDom = pred[1]
    assert got["b_test3_2.wav"] == [1.0, 1.0, 7.0]                                  # -0.3 -> clamp at 1; 1.2 -> clamp at 7 (in EmoDom)
    assert got["long_test3.wav"] == [7.0, 7.0, 1.0]
    assert got["z_test3_9.wav"] == [f(0.1), f(0.3), f(0.2)]


def test_a_corrupt_wav_leaves_the_other_rows(corpus, capsys):
    (corpus["wav_dir"] / "broken_test3.wav").write_bytes(b"RIFF\x00\x00\x00\x00WAVEjunk")
    _run("cat", corpus, CAT_TABLE)
    out = capsys.readouterr().out
    assert f"Failed to process {corpus['wav_dir'] / 'broken_test3.wav'}" in out
    assert "4 rows written" in out and "1 files failed" in out
    assert [r[0] for r in _read_csv(corpus)[1:]] == ["a_test3_1.wav", "b_test3_2.wav", "long_test3.wav", "z_test3_9.wav"]


def test_world_size_2_is_refused(corpus, capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    _run("cat", corpus, CAT_TABLE)
    assert "single-GPU" in capsys.readouterr().out
    assert not os.path.exists(os.path.join(corpus["model"], "results"))


@pytest.mark.parametrize("damage", ["truncated_pt", "pickle_not_a_pair"])
def test_a_damaged_model_directory_is_a_set_up_error_not_a_traceback(corpus, capsys, damage):
    d = _save_model_dir(corpus["model"], D=768, H=96)
    if damage == "truncated_pt":
        with open(os.path.join(d, "final_pool.pt"), "r+b") as f:
            f.truncate(100)
    else:
        with open(os.path.join(d, "train_norm_stat.pkl"), "wb") as f:
            pickle.dump(0.5, f)
    rc = BL.run_eval_cat(["--ssl_type", "wavlm-base", "--model_path", d, "--config_path", corpus["cfg"], "--head_dim", "96"],
                         predictor_factory=BL._build_predictor)       # the real set-up; it fails before anything touches a GPU
    out = capsys.readouterr().out
    assert rc == 0 and "cannot build the model" in out and "Something went wrong" in out
    assert not os.path.exists(os.path.join(d, "results"))


def test_the_label_file_is_not_read(corpus):
    """the config names a label file that does not exist: the run above succeeds anyway (eval_cat_ser.py builds class weights from it
    and never uses them)"""
    _run("cat", corpus, CAT_TABLE)
    assert len(_read_csv(corpus)) == 5


# ------------------------------------------------------------------------------- launchers (no GPU: validation comes first)
def test_new_launchers_validate_arguments(built_library):
    from interspeech_ser_amd import _lib
    lib = _lib.lib
    assert lib.ser_asp_pool_v(None, None) < 0 and b"ser_asp_pool: null pointer" in lib.ser_last_error()
    assert lib.ser_mlp_head_v(None, None) < 0 and b"ser_mlp_head: null pointer" in lib.ser_last_error()
    a = _lib.AspPoolArgs()
    assert lib.ser_asp_pool_v(ctypes.byref(a), None) < 0 and b"ser_asp_pool: null pointer" in lib.ser_last_error()
    a.x, a.hlin, a.a, a.frame_offs, a.scores, a.out = 256, 512, 768, 1024, 1280, 1536        # never dereferenced
    a.ldx, a.ldh, a.ldo, a.B, a.rows, a.max_frames = 64, 64, 128, 2, 10, 7
    a.D = 62
    assert lib.ser_asp_pool_v(ctypes.byref(a), None) == -2 and b"D=62" in lib.ser_last_error()
    a.D, a.max_frames = 64, 11
    assert lib.ser_asp_pool_v(ctypes.byref(a), None) == -2 and b"max_frames=11" in lib.ser_last_error()
    a.max_frames, a.ldo = 7, 100
    assert lib.ser_asp_pool_v(ctypes.byref(a), None) == -2 and b"ldo=100" in lib.ser_last_error()
    h = _lib.MlpHeadArgs()
    assert lib.ser_mlp_head_v(ctypes.byref(h), None) < 0 and b"ser_mlp_head: null pointer" in lib.ser_last_error()
    h.p, h.W1, h.b1, h.gamma, h.beta, h.W2, h.b2, h.hidden, h.out = (256 * i for i in range(1, 10))
    h.ldp, h.B, h.K, h.H, h.eps = 128, 2, 128, 96, 1e-5
    h.n_out = 9
    assert lib.ser_mlp_head_v(ctypes.byref(h), None) == -2 and b"n_out=9" in lib.ser_last_error()
    h.n_out, h.K = 8, 126
    assert lib.ser_mlp_head_v(ctypes.byref(h), None) == -2 and b"K=126" in lib.ser_last_error()
