"""GPU: the entry points each bridge back end launches, in order.  ``ops._call`` is wrapped to record the name of every
C-ABI function it is asked for; the expected lists below were recorded with this file on the commit before the bridges
were consolidated (one prologue interface, one back-end table), so they pin the number and the order of launches across
that change and any later one.  B = 3 is the smallest batch at which a launch per sample and a launch per batch give
different counts; "des_batch" is run both above and below DES_BATCH_DEVICE_MIN_B (kernel / host mirror, which launches
nothing)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gan_des_midi_music_gen_amd import matrix_sim_process as msp, ops  # noqa: E402

DEV = torch.device("cuda")
HERE = os.path.dirname(os.path.abspath(__file__))
B = 3

CASES = [("des", None), ("des_batch", 1), ("des_batch", 10 ** 9), ("des_device", None)]
IDS = ["des", "des_batch-kernel", "des_batch-host", "des_device"]

_MEL = ["gdm_des_log_to_notes", "gdm_synth_frames", "gdm_gemm", "gdm_power_spectrum", "gdm_gemm", "gdm_power_to_db"]
MIDI_LAUNCHES = {
    "des": ["gdm_des_scan", "gdm_des_routing", "gdm_des_routing", "gdm_des_routing", "gdm_des_log_to_roll"],
    "des_batch-kernel": ["gdm_des_scan", "gdm_des_routing", "gdm_des_run_batch", "gdm_des_log_to_roll"],
    "des_batch-host": ["gdm_des_scan", "gdm_des_routing", "gdm_des_log_to_roll"],
    "des_device": ["gdm_des_scan", "gdm_des_draws", "gdm_des_routing", "gdm_des_run_batch", "gdm_des_log_to_roll"],
}
WAV_LAUNCHES = {
    "des": ["gdm_des_scan", "gdm_des_routing", "gdm_des_routing", "gdm_des_routing"] + _MEL,
    "des_batch-kernel": ["gdm_des_scan", "gdm_des_routing", "gdm_des_run_batch"] + _MEL,
    "des_batch-host": ["gdm_des_scan", "gdm_des_routing"] + _MEL,
    "des_device": ["gdm_des_scan", "gdm_des_draws", "gdm_des_routing", "gdm_des_run_batch"] + _MEL,
}


def _fixture():
    return np.load(os.path.join(HERE, "golden", "des_prologue_rng.npz"))


@pytest.fixture
def launches(monkeypatch):
    names = []
    call = ops._call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)
    monkeypatch.setattr(ops, "_call", recording)
    return names


def _min_b(monkeypatch, min_b):
    if min_b is not None:
        monkeypatch.setattr(msp, "DES_BATCH_DEVICE_MIN_B", min_b)


@pytest.mark.parametrize("case,ident", zip(CASES, IDS), ids=IDS)
def test_matrix_to_midi_launches(case, ident, launches, monkeypatch):
    d = _fixture()
    g1 = torch.from_numpy(np.ascontiguousarray(d["midi/g1"][:B, :18, :18])).unsqueeze(1).to(DEV)
    g2 = torch.from_numpy(d["midi/g2"][:B].copy()).to(DEV)
    _min_b(monkeypatch, case[1])
    np.random.seed(21)
    rolls, _failed = msp.matrix_to_midi(g1, g2, adj_size=(18, 18), instrument=None, start=100, end=150, count=1,
                                        simulate=case[0], return_tensor=True)
    assert rolls.shape == (B, 2, 128, 50)
    print(ident, launches)
    assert launches == MIDI_LAUNCHES[ident]


@pytest.mark.parametrize("case,ident", zip(CASES, IDS), ids=IDS)
def test_matrix_to_wav_launches(case, ident, launches, monkeypatch):
    m = torch.from_numpy(_fixture()["wav/matrices"][:B]).to(DEV)
    _min_b(monkeypatch, case[1])
    np.random.seed(33)
    mel = msp.matrix_to_wav(m, size=20, start=0, end=216, device=DEV, simulate=case[0])
    assert mel.shape == (B, 128, 216)
    print(ident, launches)
    assert launches == WAV_LAUNCHES[ident]
