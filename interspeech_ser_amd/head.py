"""The consumer of the extraction path: the reference's bimodal fusion head, its training and its evaluation loop
(next row 8f-2 / BASELINE configs[4]: "HuBERT-xlarge + RoBERTa-large bimodal extract ... feeding
train_cat_bimodal_lazy_1head.py end-to-end").

Counterpart of /root/reference/bin/train_cat_bimodal_lazy_1head.py and bin/eval_cat_bimodal_lazy_1head.py as importable
functions (the reference scripts run at import time and pull ``benchmark.utils`` -> librosa / parselmouth, neither of which
this path needs): same config keys, same label / text CSV handling, same dataset item (``<lazy dir>/<wav name>.pt`` through a
bare ``torch.load``), same ``pad_sequence`` collate, same module names (the 42 state-dict keys of the reference's
``multimodal_ser.pt``), same optimiser / schedule / losses / model-selection rule, same ``results/dev.csv``.

Host code on PyTorch-ROCm (autograd, MIOpen's GRU): the head is 12 M parameters and trains in minutes; the kernels of this
repository are on the extraction side, which writes the files this module reads.
"""
from __future__ import annotations

import json
import logging
import math
import os
import random
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils.rnn import pad_sequence
from torch.utils.data import DataLoader, Dataset, WeightedRandomSampler

from .batchloop import close_logger, run_or_each, write_result_csv

CLASSES = ["Angry", "Sad", "Happy", "Surprise", "Fear", "Disgust", "Contempt", "Neutral"]      # train script :147
CLASS_LETTERS = ["A", "S", "H", "U", "F", "D", "C", "N"]                                        # eval script :129


def set_deterministic(seed: int = 42) -> None:
    """train script :45-65"""
    os.environ["PYTHONHASHSEED"] = str(seed)
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    print(f"Random seed set to: {seed}")


class CosineAnnealingScheduler(torch.optim.lr_scheduler._LRScheduler):
    """closed-form cosine schedule stepped once per epoch (train script :25-43)"""

    def __init__(self, optimizer, T_max, eta_min=0.0, last_epoch=-1):
        self.T_max, self.eta_min = T_max, eta_min
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        return [self.eta_min + (base - self.eta_min) * (1 + math.cos(math.pi * self.last_epoch / self.T_max)) / 2
                for base in self.base_lrs]


class FocalLoss(nn.Module):
    """src/losses/loss.py:7-32 with the arguments the train script uses (alpha = 1, gamma = 2, mean)"""

    def __init__(self, alpha=1.0, gamma=2.0, reduction="mean", dynamic_alpha=False):
        super().__init__()
        self.alpha, self.gamma, self.reduction, self.dynamic_alpha = alpha, gamma, reduction, dynamic_alpha

    def forward(self, preds, targets):
        probs = torch.softmax(preds, dim=1)
        pt = probs[torch.arange(targets.size(0)), targets]
        ce = -torch.log(pt + 1e-8)
        alpha = (1 - pt) if self.dynamic_alpha else self.alpha
        fl = alpha * (1 - pt) ** self.gamma * ce
        return fl.mean() if self.reduction == "mean" else (fl.sum() if self.reduction == "sum" else fl)


def ce_weight_category(pred, lab, weights):
    """benchmark/utils/loss_manager.py:85-87 (``lab``: class indices in training, the float label rows in validation)"""
    return nn.CrossEntropyLoss(weight=weights)(pred, lab)


def collate_fn(batch: List[Dict]) -> Dict:
    """train script :181-207 (+ the ``utt`` list of the eval script :138-160)"""
    out = {"feat1": pad_sequence([b["feat1"] for b in batch], batch_first=True),
           "feat2": pad_sequence([b["feat2"] for b in batch], batch_first=True)}
    if "feat3" in batch[0]:                                            # the trimodal scripts' third stream
        out["feat3"] = pad_sequence([b["feat3"] for b in batch], batch_first=True)
    if "label" in batch[0]:                                            # the test-set scoring scripts carry none
        out["label"] = torch.stack([b["label"] for b in batch])
    if "utt" in batch[0]:
        out["utt"] = [b["utt"] for b in batch]
    return out


class MultiLabelAudioDataset(Dataset):
    """train script :209-234: one item = the two feature files the extraction drivers wrote for a wav name"""

    def __init__(self, wav_files, labels, lazy_path1, lazy_path2, with_utt: bool = False, lazy_path3: Optional[str] = None):
        self.wav_paths, self.labels = list(wav_files), labels          # labels None: the test-set scoring scripts
        self.lazy_path1, self.lazy_path2, self.lazy_path3 = lazy_path1, lazy_path2, lazy_path3
        self.with_utt = with_utt
        self.verbose_one = True

    def __len__(self):
        return len(self.wav_paths)

    def __getitem__(self, idx):
        name = self.wav_paths[idx].replace(".wav", ".pt")
        paths = [os.path.join(d, name) for d in (self.lazy_path1, self.lazy_path2, self.lazy_path3) if d is not None]
        if self.verbose_one:
            print(*paths)
            self.verbose_one = False
        item = {f"feat{i + 1}": torch.load(f) for i, f in enumerate(paths)}
        if self.labels is not None:
            item["label"] = torch.tensor(self.labels[idx], dtype=torch.float)
        if self.with_utt:
            item["utt"] = self.wav_paths[idx]
        return item


class MultiModalEmotionClassifier(nn.Module):
    """train script :236-334.  Attribute names are the state-dict keys of the reference's checkpoints."""

    def __init__(self, features1_dim=1024, features2_dim=768, fusion_hidden_dim=512, num_emotions=8, dropout=0.5):
        super().__init__()
        h = fusion_hidden_dim
        self.speech_projection = nn.Linear(features1_dim, h)
        self.text_projection = nn.Linear(features2_dim, h)
        self.speech_norm = nn.LayerNorm(h)
        self.text_norm = nn.LayerNorm(h)
        self.speech_gru = nn.GRU(h, h, batch_first=True, bidirectional=True)
        self.text_gru = nn.GRU(h, h, batch_first=True, bidirectional=True)
        self.speech_attention = nn.MultiheadAttention(h * 2, 1, dropout=dropout, batch_first=True)
        self.text_attention = nn.MultiheadAttention(h * 2, 1, dropout=dropout, batch_first=True)
        self.speech_attn = nn.Linear(h * 2, 1)
        self.text_attn = nn.Linear(h * 2, 1)
        self.classifier = nn.Sequential(nn.Linear(h * 4, h), nn.ReLU(), nn.Dropout(dropout), nn.Linear(h, num_emotions))
        self.layer_norm = nn.LayerNorm(h * 4)

    @staticmethod
    def attention_pool(features, attention_layer):
        w = F.softmax(attention_layer(features), dim=1)              # [batch, seq, 1]; padded frames take part, as in the reference
        return (features * w).sum(dim=1)

    def forward(self, features1, features2):
        speech = self.speech_norm(self.speech_projection(features1))
        text = self.text_norm(self.text_projection(features2))
        speech_hidden, _ = self.speech_gru(speech)
        text_hidden, _ = self.text_gru(text)
        speech_att, _ = self.speech_attention(speech_hidden, text_hidden, text_hidden)
        text_att, _ = self.text_attention(text_hidden, speech_hidden, speech_hidden)
        speech_pooled = self.attention_pool(speech_hidden + speech_att, self.speech_attn)
        text_pooled = self.attention_pool(text_hidden + text_att, self.text_attn)
        return self.classifier(self.layer_norm(torch.cat([speech_pooled, text_pooled], dim=-1)))


class TrimodalEmotionClassifier(nn.Module):
    """The trimodal head of the reference (train_cat_trimodal_lazy_1head.py, its ``MultiModalEmotionClassifier``): speech, text and a
    third feature stream under the ``prosody_*`` names.  Each attention module serves both pairs of its query side; ``prosody_attention``
    has two heads.  Attribute names and their order are the state-dict keys of the reference's checkpoints."""

    def __init__(self, features1_dim=1024, features2_dim=768, features3_dim=1024, fusion_hidden_dim=512, num_emotions=8, dropout=0.5):
        super().__init__()
        h = fusion_hidden_dim
        self.speech_projection = nn.Linear(features1_dim, h)
        self.text_projection = nn.Linear(features2_dim, h)
        self.prosody_projection = nn.Linear(features3_dim, h)
        self.speech_norm = nn.LayerNorm(h)
        self.text_norm = nn.LayerNorm(h)
        self.prosody_norm = nn.LayerNorm(h)
        self.speech_gru = nn.GRU(h, h, batch_first=True, bidirectional=True)
        self.text_gru = nn.GRU(h, h, batch_first=True, bidirectional=True)
        self.prosody_gru = nn.GRU(h, h, batch_first=True, bidirectional=True)
        self.speech_attention = nn.MultiheadAttention(h * 2, 1, dropout=dropout, batch_first=True)
        self.text_attention = nn.MultiheadAttention(h * 2, 1, dropout=dropout, batch_first=True)
        self.prosody_attention = nn.MultiheadAttention(h * 2, 2, dropout=dropout, batch_first=True)
        self.speech_attn = nn.Linear(h * 2, 1)
        self.text_attn = nn.Linear(h * 2, 1)
        self.prosody_attn = nn.Linear(h * 2, 1)
        self.classifier = nn.Sequential(nn.Linear(h * 6, h), nn.ReLU(), nn.Dropout(dropout), nn.Linear(h, num_emotions))
        self.layer_norm = nn.LayerNorm(h * 6)

    attention_pool = staticmethod(MultiModalEmotionClassifier.attention_pool)

    def forward(self, features1, features2, prosody_features):
        hid = []
        for name, x in (("speech", features1), ("text", features2), ("prosody", prosody_features.squeeze(-1))):
            x = getattr(self, f"{name}_norm")(getattr(self, f"{name}_projection")(x))
            hid.append(getattr(self, f"{name}_gru")(x)[0])
        pooled = []
        for i, name in enumerate(("speech", "text", "prosody")):
            att, final = getattr(self, f"{name}_attention"), hid[i]
            for j in range(3):                                         # hidden + the two attended sequences, in the reference's order
                if j != i:
                    final = final + att(hid[i], hid[j], hid[j])[0]
            pooled.append(self.attention_pool(final, getattr(self, f"{name}_attn")))
        return self.classifier(self.layer_norm(torch.cat(pooled, dim=-1)))


def macro_f1(labels: Sequence[int], preds: Sequence[int]) -> float:
    """sklearn.metrics.f1_score(labels, preds, average='macro'): mean F1 over the classes present in labels or preds
    (a class with no true and no predicted sample is left out; 0/0 counts as 0)."""
    labels, preds = np.asarray(labels, dtype=np.int64), np.asarray(preds, dtype=np.int64)
    scores = []
    for c in np.union1d(labels, preds):
        tp = float(np.sum((preds == c) & (labels == c)))
        fp = float(np.sum((preds == c) & (labels != c)))
        fn = float(np.sum((preds != c) & (labels == c)))
        scores.append(0.0 if 2 * tp + fp + fn == 0 else 2 * tp / (2 * tp + fp + fn))
    return float(np.mean(scores)) if scores else 0.0


def _class_weights(df, device) -> torch.Tensor:
    """total / (n_classes * frequency), 0 for an absent class (train script :150-161)"""
    freq = df[CLASSES].sum().to_dict()
    total = len(df)
    return torch.tensor([total / (len(CLASSES) * freq[c]) if freq[c] != 0 else 0 for c in CLASSES], device=device, dtype=torch.float)


def _logger(model_path: str) -> logging.Logger:
    log = logging.getLogger(f"ser_head.{model_path}.{time.time()}")
    log.setLevel(logging.INFO)
    log.propagate = False
    fmt = logging.Formatter("%(asctime)s - %(levelname)s - %(message)s")
    for h in (logging.FileHandler(os.path.join(model_path, "%s-%d.log" % ("loggingtxt", time.time()))), logging.StreamHandler()):
        h.setFormatter(fmt)
        log.addHandler(h)
    return log


def _frames(config: Dict):
    import pandas as pd
    label_df, text_df = pd.read_csv(config["label_path"]), pd.read_csv(config["txt_dir"])
    return label_df.merge(text_df, on="FileName", how="left")


def _device(name: Optional[str]) -> torch.device:
    return torch.device(name) if name else torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _model(config: Dict, device, modalities: int = 2, hidden: int = 512) -> nn.Module:
    """the head the reference's scripts build (fusion_hidden_dim=512 there; ``score`` passes the checkpoint's own width)"""
    if modalities == 3:
        return TrimodalEmotionClassifier(features1_dim=config["feat1_dim"], features2_dim=config["feat2_dim"], features3_dim=config["feat3_dim"],
                                         fusion_hidden_dim=hidden, num_emotions=8, dropout=0.5).to(device)
    if modalities != 2:
        raise ValueError(f"modalities must be 2 or 3, got {modalities!r}")
    return MultiModalEmotionClassifier(features1_dim=config["feat1_dim"], features2_dim=config["feat2_dim"],
                                       fusion_hidden_dim=hidden, num_emotions=8, dropout=0.5).to(device)


def _inputs(batch: Dict, device) -> list:
    """the model's arguments from a collated batch: feat1, feat2 (, feat3)"""
    return [batch[k].to(device) for k in ("feat1", "feat2", "feat3") if k in batch]


def _validate(model, loader, device):
    """one pass over the Development split (train script :447-476, eval script :310-341)"""
    model.eval()
    logits_all, labels_all, preds, gold, utts = [], [], [], [], []
    for batch in loader:
        labels = batch["label"].to(device)
        with torch.no_grad():
            logits = model(*_inputs(batch, device))
        logits_all.append(logits)
        labels_all.append(labels)
        preds.extend(torch.argmax(logits, dim=1).cpu().numpy())
        gold.extend(batch["label"].max(dim=1)[1].numpy())
        utts.extend(batch.get("utt", []))
    return torch.cat(logits_all, 0), torch.cat(labels_all, 0), preds, gold, utts


def train(config: Dict, seed: int = 7, device: Optional[str] = None, modalities: int = 2) -> Dict:
    """bin/train_cat_bimodal_lazy_1head.py (``modalities=3``: bin/train_cat_trimodal_lazy_1head.py, with ``lazy_dir3`` / ``feat3_dim``) as a
    function.  Returns {"best_f1", "best_epoch", "model_file", "history"}."""
    set_deterministic(seed)
    dev = _device(device)
    batch_size, accum = config["batch_size"], config["accum_step"]
    assert accum > 0 and batch_size % accum == 0
    epochs, lr, model_path = config["epochs"], config["lr"], config["model_path"]
    os.makedirs(model_path, exist_ok=True)
    balanced = bool(config.get("use_balanced_batch", False))
    focal = bool(config.get("use_focalloss", False))
    log = _logger(model_path)
    log.info(f"Starting an Lazy OwnSermodel wavlm-based experiment in model path = {model_path}")
    log.info(f"Using LR = {lr} Epochs = {epochs} Batch size = {batch_size} Accum steps = {accum}")
    log.info(f"Using balanced batch = {balanced}")
    log.info(f"Using focalloss = {focal}")

    df = _frames(config)
    train_df, val_df = df[df["Split_Set"] == "Train"], df[df["Split_Set"] == "Development"]
    w_train, w_val = _class_weights(train_df, dev), _class_weights(val_df, dev)
    log.info(f"Class weights: {w_train}")
    lazy3 = config["lazy_dir3"] if modalities == 3 else None
    train_ds = MultiLabelAudioDataset(train_df["FileName"].tolist(), train_df[CLASSES].values, config["lazy_dir1"], config["lazy_dir2"], lazy_path3=lazy3)
    val_ds = MultiLabelAudioDataset(val_df["FileName"].tolist(), val_df[CLASSES].values, config["lazy_dir1"], config["lazy_dir2"], lazy_path3=lazy3)
    if balanced:                                                       # train script :340-361
        log.info("Using balanced batch. Computing sample weights...")
        freq = train_df[CLASSES].sum().to_dict()
        cw = {c: 1 / f if f != 0 else 0 for c, f in freq.items()}
        factor = len(cw) / sum(cw.values())
        cw = {c: w * factor for c, w in cw.items()}
        sample_w = [cw[train_df[CLASSES].iloc[i].idxmax()] for i in range(len(train_df))]
        sampler = WeightedRandomSampler(weights=sample_w, num_samples=len(train_ds), replacement=True)
        train_loader = DataLoader(train_ds, batch_size=batch_size, sampler=sampler, collate_fn=collate_fn)
    else:
        train_loader = DataLoader(train_ds, batch_size=batch_size, shuffle=True, collate_fn=collate_fn)
    val_loader = DataLoader(val_ds, batch_size=batch_size, collate_fn=collate_fn)

    model = _model(config, dev, modalities)
    optimizer = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=1e-6)
    scheduler = CosineAnnealingScheduler(optimizer, T_max=epochs, eta_min=1e-6)
    focal_loss = FocalLoss(alpha=1, gamma=2, reduction="mean", dynamic_alpha=modalities == 3)     # the trimodal script passes True
    best = {"best_f1": 0.0, "best_epoch": 0, "best_loss": 1e10, "model_file": os.path.join(model_path, "multimodal_ser.pt"), "history": []}
    log.info("Starting training...")
    for epoch in range(epochs):
        print("Epoch: ", epoch)
        model.train()
        n_batches = len(train_loader)
        for cnt, batch in enumerate(train_loader):
            y = batch["label"].max(dim=1)[1].to(dev).long()
            optimizer.zero_grad()                                      # per batch, as the reference does (:413)
            logits = model(*_inputs(batch, dev))
            loss = ce_weight_category(logits, y, None if balanced else w_train)
            total = (focal_loss(logits, y) if focal else loss) / accum
            total.backward()
            if (cnt + 1) % accum == 0 or (cnt + 1) == n_batches:
                optimizer.step()
            if (cnt + 2) % 200 == 0:
                log.info(f"Epoch ({epoch + 1}/{epochs})| step = {cnt + 1}: loss = {loss} current lr = {scheduler.get_last_lr()[0]}")
        scheduler.step()
        logits_all, labels_all, preds, gold, _ = _validate(model, val_loader, dev)
        dev_loss = ce_weight_category(logits_all, labels_all, w_val)
        f1 = macro_f1(gold, preds)
        log.info(f"|VALIDATION| Epoch ({epoch + 1}/{epochs}): eval_loss = {dev_loss} eval f1 = {f1}")
        best["history"].append({"epoch": epoch + 1, "eval_loss": float(dev_loss), "eval_f1": f1})
        if best["best_f1"] < f1:
            log.info(f"New best model at epoch {epoch + 1}")
            best.update(best_f1=f1, best_epoch=epoch, best_loss=float(dev_loss))
            print("Save", epoch)
            print("Loss", float(dev_loss))
            torch.save(model.state_dict(), best["model_file"])
    close_logger(log)
    return best


def evaluate(config: Dict, seed: int = 7, device: Optional[str] = None, engine: str = "torch", mode: str = "f16x", modalities: int = 2) -> Dict:
    """bin/eval_cat_bimodal_lazy_1head.py as a function: Development split through ``multimodal_ser.pt``, macro-F1,
    ``<model_path>/results/dev.csv`` (Filename, Prediction letter, the 8 logits as class_i_prob).
    ``engine="torch"`` (default): the PyTorch module, batches of ``config["batch_size"]`` padded to their longest utterance (padded frames
    take part, as in the reference's class).  ``engine="hip"``: the head as kernels of this library (engine.FusionHead), 16 files at a
    time as packed ragged batches -- every utterance alone, the arithmetic of the reference's own evaluation loop (``batch_size=1``).
    ``modalities=3``: the trimodal head (``lazy_dir3`` / ``feat3_dim``; engine.TrimodalHead on the device)."""
    if modalities not in (2, 3):
        raise ValueError(f"modalities must be 2 or 3, got {modalities!r}")
    if engine == "hip":
        return _evaluate_hip(config, seed, device, mode, modalities)
    if engine != "torch":
        raise ValueError(f"engine must be 'torch' or 'hip', got {engine!r}")
    set_deterministic(seed)
    dev = _device(device)
    model_path = config["model_path"]
    os.makedirs(model_path, exist_ok=True)
    log = _logger(model_path)
    df = _frames(config)
    val_df = df[df["Split_Set"] == "Development"]
    val_ds = MultiLabelAudioDataset(val_df["FileName"].tolist(), val_df[CLASSES].values, config["lazy_dir1"], config["lazy_dir2"], with_utt=True,
                                    lazy_path3=config["lazy_dir3"] if modalities == 3 else None)
    val_loader = DataLoader(val_ds, batch_size=config["batch_size"], collate_fn=collate_fn)
    model = _model(config, dev, modalities)
    model.load_state_dict(torch.load(os.path.join(model_path, "multimodal_ser.pt"), map_location=dev), strict=False)
    log.info("Starting evaluation...")
    logits_all, labels_all, preds, gold, utts = _validate(model, val_loader, dev)
    loss = ce_weight_category(logits_all, labels_all, None)
    f1 = macro_f1(gold, preds)
    log.info(f"|Metrics| eval_loss = {loss} eval f1 = {f1}")
    csv_file = write_result_csv(model_path, "dev", "Filename", utts, logits_all.cpu().numpy(), CLASS_LETTERS)
    close_logger(log)
    return {"eval_loss": float(loss), "eval_f1": f1, "csv": csv_file, "n": len(utts)}


HIP_BATCH = 16                      # files per packed ragged batch of the "hip" engine (one MFMA column group of ser_gru_v)
NO_CPU_PATH = "Error: no MI355X visible -- this build has no CPU path (the CPU oracle under oracle/ is test-only)"


def _hip_head(config: Dict, dev, mode: str, modalities: int):
    """engine.FusionHead / engine.TrimodalHead over ``<model_path>/multimodal_ser.pt`` (keys beyond the head's own -- a ranking checkpoint's
    second classifier -- are ignored: the ranking scoring scripts throw that output away)"""
    from .engine import FusionHead, TrimodalHead
    sd = torch.load(os.path.join(config["model_path"], "multimodal_ser.pt"), map_location="cpu", weights_only=True)
    if modalities == 3:
        return TrimodalHead(sd, config["feat1_dim"], config["feat2_dim"], config["feat3_dim"], dev, mode)
    return FusionHead(sd, config["feat1_dim"], config["feat2_dim"], dev, mode)


def _run_hip(head, config: Dict, names: Sequence[str], dev, modalities: int):
    """``names`` through the head on the device, HIP_BATCH files per packed ragged batch -> (indices of the files done, their logit rows,
    number of files failed).  A batch whose range-guard word or ser_gru_v error word is set, or whose forward raises, goes through
    ``batchloop.run_or_each``: retried file by file, and a file that still fails gets a printed line and no row."""
    lazy = [config[f"lazy_dir{i + 1}"] for i in range(modalities)]
    done, rows, failed = [], [], 0

    def fail(name, err):
        nonlocal failed
        failed += 1
        print(f"Failed to process {name}: {err}")

    def run(items):
        """items: (index, name, features...) -> error message or None; appends the rows of a clean batch"""
        args = []
        for m in range(modalities):
            args.append(torch.cat([it[2 + m] for it in items]).to(dev))
            args.append(np.concatenate([[0], np.cumsum([it[2 + m].shape[0] for it in items])]))
        out = head.forward(*args).cpu().numpy().copy()
        err = head.failure(*head.status())
        if err is None:
            for it, row in zip(items, out):
                done.append(it[0])
                rows.append(row)
        return err

    first = True
    for i in range(0, len(names), HIP_BATCH):
        items = []
        for k, name in enumerate(names[i:i + HIP_BATCH]):
            pt = name.replace(".wav", ".pt")
            files = [os.path.join(d, pt) for d in lazy]
            if first:
                print(*files)
                first = False
            try:
                feats = [torch.load(f, weights_only=True) for f in files]
                if modalities == 3 and feats[2].dim() == 3 and feats[2].shape[-1] == 1:
                    feats[2] = feats[2].squeeze(-1)            # the reference squeezes the third stream's last axis
                if any(a.dim() != 2 or a.shape[0] < 1 for a in feats):
                    raise ValueError("feature files must hold [T >= 1, D] matrices, got " + " and ".join(str(tuple(a.shape)) for a in feats))
                items.append((i + k, name, *[a.float().contiguous() for a in feats]))
            except Exception as e:                              # noqa: BLE001  (per-file failure, as in the extraction drivers)
                fail(name, e)
        if items:
            run_or_each(items, run, lambda it, e: fail(it[1], e))
    return done, rows, failed


def _evaluate_hip(config: Dict, seed: int, device: Optional[str], mode: str, modalities: int = 2) -> Dict:
    """``evaluate`` with the head on the device (``_run_hip``)."""
    if not torch.cuda.is_available():
        print(NO_CPU_PATH)
        return {"eval_loss": None, "eval_f1": None, "csv": None, "n": 0, "failed": 0}
    set_deterministic(seed)
    dev = torch.device(device or "cuda:0")
    model_path = config["model_path"]
    os.makedirs(model_path, exist_ok=True)
    log = _logger(model_path)
    df = _frames(config)
    val_df = df[df["Split_Set"] == "Development"]
    names, labels = val_df["FileName"].tolist(), val_df[CLASSES].values
    head = _hip_head(config, dev, mode, modalities)
    log.info("Starting evaluation...")
    idx, rows, failed = _run_hip(head, config, names, dev, modalities)
    done, gold = [names[i] for i in idx], [labels[i] for i in idx]
    loss, f1 = float("nan"), 0.0
    if rows:
        logits_all = torch.from_numpy(np.stack(rows))
        labels_all = torch.tensor(np.stack(gold), dtype=torch.float)
        loss = float(ce_weight_category(logits_all, labels_all, None))
        f1 = macro_f1(labels_all.max(dim=1)[1].numpy(), torch.argmax(logits_all, dim=1).numpy())
    log.info(f"|Metrics| eval_loss = {loss} eval f1 = {f1}")
    csv_file = write_result_csv(model_path, "dev", "Filename", done, rows, CLASS_LETTERS)
    print(f"{len(done)} rows written, {failed} files failed")
    close_logger(log)
    return {"eval_loss": loss, "eval_f1": f1, "csv": csv_file, "n": len(done), "failed": failed}


TEST_CSV = "./test/Categorical_test.csv"


def score(config: Dict, seed: int = 7, device: Optional[str] = None, engine: str = "torch", mode: str = "f16x", modalities: int = 2,
          test_csv: str = TEST_CSV) -> Dict:
    """The reference's four bin/test_cat_{bi,tri}modal_lazy_stacking_1head[_ranking].py as one function: the ``FileName`` column of
    ``test_csv`` through ``<model_path>/multimodal_ser.pt`` -- no labels -- into ``<model_path>/results/test.csv`` (FileName, Prediction
    letter, the 8 logits as class_i_prob; the file the stacking step and the submission read).  A ranking checkpoint is the plain head with a
    second classifier in its state dict, whose output those scripts throw away: the extra keys are ignored.
    ``engine="torch"``: the PyTorch module, one file at a time (``batch_size=1``, as the reference).  ``engine="hip"``: the head as kernels of
    this library, 16 files per packed ragged batch -- the same arithmetic, every utterance alone.
    Returns {"csv", "n", "failed"}."""
    if modalities not in (2, 3):
        raise ValueError(f"modalities must be 2 or 3, got {modalities!r}")
    if engine not in ("torch", "hip"):
        raise ValueError(f"engine must be 'torch' or 'hip', got {engine!r}")
    if engine == "hip" and not torch.cuda.is_available():
        print(NO_CPU_PATH)
        return {"csv": None, "n": 0, "failed": 0}
    import pandas as pd
    set_deterministic(seed)
    model_path = config["model_path"]
    os.makedirs(model_path, exist_ok=True)
    log = _logger(model_path)
    names = pd.read_csv(test_csv)["FileName"].tolist()
    failed = 0
    if engine == "hip":
        dev = torch.device(device or "cuda:0")
        head = _hip_head(config, dev, mode, modalities)
        log.info("Starting scoring test samples...")
        idx, rows, failed = _run_hip(head, config, names, dev, modalities)
        done = [names[i] for i in idx]
    else:
        dev = _device(device)
        ds = MultiLabelAudioDataset(names, None, config["lazy_dir1"], config["lazy_dir2"], with_utt=True,
                                    lazy_path3=config["lazy_dir3"] if modalities == 3 else None)
        loader = DataLoader(ds, batch_size=1, collate_fn=collate_fn)
        sd = torch.load(os.path.join(model_path, "multimodal_ser.pt"), map_location=dev, weights_only=True)
        model = _model(config, dev, modalities, hidden=int(sd["speech_norm.weight"].shape[0]) if "speech_norm.weight" in sd else 512)
        missing = model.load_state_dict(sd, strict=False).missing_keys
        if missing:
            raise ValueError(f"the head's state dict lacks {missing[:4]}{' ...' if len(missing) > 4 else ''} ({len(missing)} keys)")
        model.eval()
        log.info("Starting scoring test samples...")
        rows, done = [], []
        for batch in loader:
            with torch.no_grad():
                logits = model(*_inputs(batch, dev))
            rows.extend(logits.cpu().numpy())
            done.extend(batch["utt"])
    csv_file = write_result_csv(model_path, "test", "FileName", done, rows, CLASS_LETTERS)      # "FileName" here, "Filename" in dev.csv
    if engine == "hip":
        print(f"{len(done)} rows written, {failed} files failed")
    close_logger(log)
    return {"csv": csv_file, "n": len(done), "failed": failed}


def main(argv: Optional[Sequence[str]] = None, evaluate_only: bool = False, modalities: int = 2, score_only: bool = False) -> int:
    import argparse
    p = argparse.ArgumentParser()
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--config_path", type=str, default="./configs/config_cat.json")
    if evaluate_only or score_only:                             # additive: the head as kernels of this library (engine.FusionHead / TrimodalHead)
        p.add_argument("--engine", type=str, default="torch", choices=["torch", "hip"])
        p.add_argument("--mode", type=str, default="f16x", choices=["f16x", "fp32x", "bf16"])
    if score_only:
        p.add_argument("--test_csv", type=str, default=TEST_CSV)
    args = p.parse_args(argv)
    with open(args.config_path, "r") as f:
        config = json.load(f)
    if score_only:
        score(config, seed=args.seed, engine=args.engine, mode=args.mode, modalities=modalities, test_csv=args.test_csv)
    elif evaluate_only:
        evaluate(config, seed=args.seed, engine=args.engine, mode=args.mode, modalities=modalities)
    else:
        train(config, seed=args.seed, modalities=modalities)
    return 0
