"""Drop-in surface of model 1 (GAN_DES/SIMNN.py) on MI355X.

Same public names, constructor signatures, state_dict keys and training-loop semantics as the reference module:

    get_noise(n_samples, noise_dim, device='cpu')                 SIMNN.py:37-46
    weights_init(m)                                               SIMNN.py:49-59
    Generator(no_of_channels=1, noise_dim=100, gen_dim=32)        SIMNN.py:62-112
    Discriminator(no_of_channels=1, disc_dim=32)                  SIMNN.py:115-142
    SimNN(n)                                                      SIMNN.py:145-170
    generate_song(model_folder, bridge="des")                     SIMNN.py:201-216
    des_fake_provider(start=0, end=216, batched=False)            (this build: the DES bridge as a fake provider)
    sample_matrices(gen, n_samples)                               (this build: the batched form of generate_song)
    generate_songs(model, n_samples, out_dir=...)                 (this build: n clips, each with its MIDI and WAV file)
    train(...)  /  python -m gan_des_midi_music_gen_amd.SIMNN     SIMNN.py:234-348 (the __main__ loop)

The module tree holds ordinary ``nn.ConvTranspose2d / nn.BatchNorm2d / nn.Conv2d / nn.Linear`` children purely as
parameter containers (so ``.apply(weights_init)``, ``state_dict()``, ``load_state_dict(strict=True)`` of the committed
``gen_100_*.pt`` and any ``torch.optim`` optimizer behave exactly as with the reference); their own ``forward`` is
never called -- ``forward`` here dispatches to the HIP kernels behind include/gdm.h.
"""
import os
import time

import torch
from torch import nn
import torch.nn.init as init

from . import functional as Fn
from . import matrix_sim_process as msp
from . import synthetic


def get_noise(n_samples, noise_dim, device="cpu"):
    """(n_samples, noise_dim, 1, 1) standard-normal noise on ``device``."""
    return torch.randn(n_samples, noise_dim, 1, 1, device=device)


def weights_init(m):
    """Conv2d/ConvTranspose2d weight ~ N(0, 0.02); BatchNorm2d weight ~ N(0, 0.02) (as the reference does), bias 0."""
    if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
        init.normal_(m.weight, mean=0.0, std=0.02)
    if isinstance(m, nn.BatchNorm2d):
        init.normal_(m.weight, mean=0.0, std=0.02)
        init.constant_(m.bias, val=0)


class Generator(nn.Module):
    """noise (B,noise_dim,1,1) -> DES parameter matrix (B,no_of_channels,20,20) in (0,1).

    ConvT(noise->4g,k4) BN ReLU, ConvT(4g->2g,k4,s2,p1) BN ReLU, ConvT(2g->g,k4,s2,p1) BN ReLU, ConvT(g->C,k5), sigmoid.
    """

    def __init__(self, no_of_channels=1, noise_dim=100, gen_dim=32):
        super().__init__()
        g = gen_dim
        self.conv1 = nn.ConvTranspose2d(noise_dim, g * 4, kernel_size=4, stride=1, padding=0, bias=False)
        self.conv2 = nn.ConvTranspose2d(g * 4, g * 2, kernel_size=4, stride=2, padding=1, bias=False)
        self.conv3 = nn.ConvTranspose2d(g * 2, g, kernel_size=4, stride=2, padding=1, bias=False)
        self.conv4 = nn.ConvTranspose2d(g, no_of_channels, kernel_size=5, stride=1, padding=0, bias=False)
        self.batch_norm1 = nn.BatchNorm2d(g * 4)
        self.batch_norm2 = nn.BatchNorm2d(g * 2)
        self.batch_norm3 = nn.BatchNorm2d(g)
        self.compute_dtype = None  # None -> functional.get_compute_dtype()
        self._eval_cache = {}      # the eval-mode kernel's weight pack, rebuilt when a weight changes (not module state)
        self._initialize_weights()

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.ConvTranspose2d):
                init.normal_(m.weight, 0.0, 0.02)
            elif isinstance(m, nn.BatchNorm2d):
                init.normal_(m.weight, 1.0, 0.02)
                init.constant_(m.bias, 0)

    def forward(self, input):
        dt = Fn.get_compute_dtype() if self.compute_dtype is None else Fn._NAMES[self.compute_dtype]
        bns = (self.batch_norm1, self.batch_norm2, self.batch_norm3)
        buffers = tuple((bn.running_mean, bn.running_var, bn.num_batches_tracked) for bn in bns)
        return Fn.SimnnGenFn.apply(input, self.conv1.weight, self.conv2.weight, self.conv3.weight, self.conv4.weight,
                                   bns[0].weight, bns[0].bias, bns[1].weight, bns[1].bias, bns[2].weight, bns[2].bias,
                                   buffers, self.training, dt, self._eval_cache)


def disc_feature_hw(input_hw):
    """(H, W) of the input window -> (H2, W2) of the 32-channel feature map in front of fc1."""
    h, w = input_hw
    return ((h + 1) // 2) // 2, ((w + 1) // 2) // 2


class Discriminator(nn.Module):
    """(B, H, W) mel-dB windows -> (B, 1) sigmoid scores.

    Conv(1->16,k2,p1) ReLU Pool2, Conv(16->32,k3,p1) ReLU Pool2, flatten, Linear(->128) ReLU, Linear(->1), sigmoid.
    ``input_hw`` (keyword-only, default = the reference's hard-wired 128x216 -> fc1.in_features 32*32*54) is the
    build's one extension: the benchmark config uses 128x256 windows (geometry note).
    """

    def __init__(self, no_of_channels=1, disc_dim=32, *, input_hw=(128, 216)):
        super().__init__()
        self.input_hw = tuple(input_hw)
        fh, fw = disc_feature_hw(self.input_hw)
        self.conv1 = nn.Conv2d(1, 16, kernel_size=2, stride=1, padding=1)
        self.conv2 = nn.Conv2d(16, 32, kernel_size=3, stride=1, padding=1)
        self.pool = nn.MaxPool2d(kernel_size=2, stride=2, padding=0)
        self.fc1 = nn.Linear(32 * fh * fw, 128)
        self.fc2 = nn.Linear(128, 1)
        self.compute_dtype = None

    def forward(self, input):
        dt = Fn.get_compute_dtype() if self.compute_dtype is None else Fn._NAMES[self.compute_dtype]
        return Fn.SimnnDiscFn.apply(input, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                                    self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, dt)


class SimNN(nn.Module):
    """Experimental CNN of the reference (SIMNN.py:145-198): spectrogram (B,1,H,W) -> (n x n matrix, 4 length-n
    vectors).  Never reached by the reference's training loop; kept complete for the API.

    As upstream, ``forward`` RE-CREATES ``fc1`` with fresh default-initialised weights on every call, sized to the
    flattened feature map (SIMNN.py:161: ``self.fc1 = nn.Linear(x.size(1), 512).to(x.device)`` -- drawn on the CPU
    generator, then moved), so results are reproducible only under a fixed ``torch.manual_seed`` right before the call
    (that is how tests/golden/simnn_net.npz pins it).  Convolutions run as im2col + MFMA GEMM with fused bias/ReLU,
    pooling and the dense layers on the generic kernels behind include/gdm.h.
    """

    def __init__(self, n):
        super().__init__()
        self.n = n
        self.conv1 = nn.Conv2d(1, 32, kernel_size=3, stride=1, padding=1)
        self.conv2 = nn.Conv2d(32, 64, kernel_size=3, stride=1, padding=1)
        self.fc1 = nn.Linear(64 * 32 * 32, 512)  # replaced in forward, like upstream
        self.fc2 = nn.Linear(512, self.n * self.n + 4 * self.n)
        self.compute_dtype = None

    def forward(self, x):
        dt = Fn.get_compute_dtype() if self.compute_dtype is None else Fn._NAMES[self.compute_dtype]
        feat = 64 * (x.size(2) // 4) * (x.size(3) // 4)
        self.fc1 = nn.Linear(feat, 512).to(x.device)                  # SIMNN.py:161
        output = Fn.SimnnNetFn.apply(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                                     self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, dt)
        n = self.n
        matrix = output[:, :n * n].view(-1, n, n)
        array1 = output[:, n * n:n * n + n]
        array2 = output[:, n * n + n:n * n + 2 * n]
        array3 = output[:, n * n + 2 * n:n * n + 3 * n]
        array4 = output[:, n * n + 3 * n:]
        return matrix, array1, array2, array3, array4

    @staticmethod
    def create_model(n):
        return SimNN(n)


def _load_generator(model_folder, device):
    gen = Generator()
    gen.load_state_dict(torch.load(model_folder, map_location="cpu", weights_only=True))
    return gen.to(device)


def generate_song(model_folder, device=None, bridge=None, compute_dtype=None, *, midi_path=None, wav_path=None,
                  max_seconds=None):
    """Load a generator checkpoint (same ``gen_*.pt`` files the reference writes) and emit one DES matrix.

    The reference then renders audio through ``matrix_to_wav`` (SIMNN.py:214-215).  bridge="des": the built-in bridge
    (matrix_sim_process.matrix_to_wav(simulate="des"): DES core, log -> notes, integer synth, mel) -- the (128, 216) dB
    spectrogram tensor is returned, as upstream; ``midi_path`` / ``wav_path`` also write the clip's MIDI file and its
    audio (mono 16-bit, 44 100 Hz, rendered on the device in bounded chunks; ``max_seconds`` cuts it; a blank clip is
    the reference's five seconds of silence).  bridge="des_batch": the same with the simulation on the device
    (matrix_to_wav(simulate="des_batch"); see matrix_sim_process for what differs).  bridge=callable continues from the (20,20) numpy matrix; with no bridge
    the matrix is returned.
    compute_dtype: None (the process default, exact fp32 unless changed) or "bf16" (the one-launch eval kernel).
    """
    device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    gen = _load_generator(model_folder, device).eval()
    gen.compute_dtype = compute_dtype
    with torch.no_grad():
        generated = gen(get_noise(1, 100, device=device)).detach()
    if isinstance(bridge, str):
        msp.check_back_end(bridge, "unknown bridge", ValueError)
        return _des_song(generated.reshape(1, 20, 20), midi_path, wav_path, max_seconds, bridge)
    adj = generated.squeeze().cpu().numpy()
    return bridge(adj) if bridge is not None else adj


def _write_clip(notes, n_notes, i, count, total, midi_path, wav_path, max_seconds):
    """The two files of clip i of a batch of note lists (notes, n_notes: device tensors; count = int(n_notes[i]) and
    total = int(clip_len[i]) on the host): the MIDI file of its notes and its audio, mono 16-bit at 44 100 Hz, rendered
    on the device in bounded chunks.  A blank clip is the reference's five seconds of silence; ``max_seconds`` cuts
    the audio."""
    from . import ops, sim_log_process_music as slpm, sim_log_to_midi, util
    if midi_path is not None:
        sim_log_to_midi.write_midi(slpm.notes_to_track(notes[i, :count].cpu().numpy()), midi_path)
    if wav_path is not None:
        util.write_wav_chunks(wav_path, total, lambda first, n: ops.synth_pcm(notes[i:i + 1], n_notes[i:i + 1], first, n),
                              blank=total == 0, max_seconds=max_seconds)


def _des_song(matrix, midi_path, wav_path, max_seconds, bridge):
    """matrix_to_wav with the built-in back end ``bridge`` for one matrix, keeping the note list for the two files."""
    mel, (notes, n_notes, clip_len) = msp.matrices_to_mel(matrix, simulate=bridge)
    _write_clip(notes, n_notes, 0, int(n_notes[0]), int(clip_len[0]), midi_path, wav_path, max_seconds)
    return mel[0]


class SongBatch:
    """What ``generate_songs`` returns: ``mel`` (n, 128, 216) dB on the device; ``notes`` (n, cap, 4), ``n_notes`` (n,),
    ``clip_len`` (n,): the note lists and clip lengths in samples, device tensors; ``midi_paths``, ``wav_paths``: the
    files written, None where none was."""

    def __init__(self, mel, notes, n_notes, clip_len, midi_paths, wav_paths):
        self.mel, self.notes, self.n_notes, self.clip_len = mel, notes, n_notes, clip_len
        self.midi_paths, self.wav_paths = midi_paths, wav_paths


def generate_songs(model, n_samples=None, *, noise=None, bridge="des_batch", out_dir=None, midi=True, wav=True,
                   max_seconds=None, compute_dtype="bf16", device=None):
    """``generate_song`` for a batch: n clips from a trained generator, each with its MIDI file and its audio.

    model: a ``Generator`` or the path of a ``gen_*.pt`` checkpoint.  ``sample_matrices`` draws the n matrices (one
    launch), then bridge "des_batch" simulates all of them in one device launch
    (matrix_sim_process.matrices_to_mel) and "des" keeps the reference's interleaved order
    (see matrix_sim_process for what differs); "des_device" also makes the draws on the device, one stream per clip.
    With ``out_dir`` clip i is written to ``out_dir/song_{i:04d}.mid`` (midi)
    and ``.wav`` (wav) exactly as ``generate_song`` writes its one clip; with out_dir=None nothing is written and the
    path lists hold None.  -> SongBatch."""
    msp.check_back_end(bridge, "unknown bridge", ValueError)
    matrices = sample_matrices(model, n_samples, noise=noise, compute_dtype=compute_dtype, device=device)
    n = matrices.shape[0]
    mel, (notes, n_notes, clip_len) = msp.matrices_to_mel(matrices.reshape(n, 20, 20), simulate=bridge)
    midi_paths, wav_paths = [None] * n, [None] * n
    if out_dir is not None:
        counts, lengths = n_notes.cpu(), clip_len.cpu()                  # one read-back for all clips
        for i in range(n):
            stem = os.path.join(out_dir, f"song_{i:04d}")
            midi_paths[i] = stem + ".mid" if midi else None
            wav_paths[i] = stem + ".wav" if wav else None
            _write_clip(notes, n_notes, i, int(counts[i]), int(lengths[i]), midi_paths[i], wav_paths[i], max_seconds)
    return SongBatch(mel, notes, n_notes, clip_len, midi_paths, wav_paths)


def des_fake_provider(start=0, end=216, max_events=200000, batched=False):
    """The built-in DES bridge as the ``fake`` callable of ``SimnnTrainer.step`` / ``train(fake_provider=...)``:
    generated (B,1,20,20) device tensor -> (B,128,end-start) dB tensor on the same device (SIMNN.py:301).
    batched: simulate on the device (matrix_to_wav(simulate="des_batch")); a back end's name ("des_batch",
    "des_device") selects that one."""
    simulate = batched if isinstance(batched, str) else ("des_batch" if batched else "des")

    def provider(generated):
        return msp.matrix_to_wav(generated, start=start, end=end, device=generated.device, simulate=simulate,
                                 max_events=max_events)
    return provider


def sample_matrices(gen, n_samples=None, *, noise=None, compute_dtype="bf16", device=None):
    """Draw DES parameter matrices from a trained generator: the batched form of ``generate_song``.

    gen: a ``Generator`` or the path of a ``gen_*.pt`` checkpoint (loaded as ``generate_song`` loads it).
    n_samples standard-normal noise vectors are drawn on the device, or ``noise`` (n, noise_dim[, 1, 1]) is used.
    Returns (n, 1, 20, 20) fp32 on the device, contiguous: the layout ``matrix_sim_process.wav_prologue`` /
    ``matrix_to_wav`` read in place.  The eval arithmetic (BatchNorm on its running statistics) runs whatever
    ``gen.training`` says, and no state of the module changes: parameters, running statistics,
    ``num_batches_tracked``, ``training`` and ``compute_dtype`` are as before.  compute_dtype "bf16" (default) is one
    kernel launch for the whole batch; "fp32" walks the exact layer-wise path.
    """
    if not isinstance(gen, nn.Module):
        device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        gen = _load_generator(gen, device)
    dev = gen.conv1.weight.device
    if noise is None:
        if n_samples is None:
            raise ValueError("sample_matrices needs n_samples or noise")
        noise = get_noise(int(n_samples), gen.conv1.in_channels, device=dev)
    elif n_samples is not None and int(n_samples) != noise.shape[0]:
        raise ValueError(f"n_samples = {n_samples} but noise holds {noise.shape[0]} vectors")
    noise = noise.to(dev).reshape(noise.shape[0], -1, 1, 1)
    bns = (gen.batch_norm1, gen.batch_norm2, gen.batch_norm3)
    ws = [m.weight.detach() for m in (gen.conv1, gen.conv2, gen.conv3, gen.conv4)]
    args = [(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.num_batches_tracked) for bn in bns]
    dt = Fn._NAMES[compute_dtype]
    out, _ = Fn.simnn_gen_forward(noise, ws, args, False, dt, need_backward=False,
                                  cache=gen._eval_cache if Fn._gen_eval_ok(ws, False, dt) else None)
    return out.contiguous()


def _song_batches(spec, batch_size, shuffle):
    """One epoch over the (N, H, W) windows of a song as ``DataLoader(batch_size, shuffle)`` deals them: the last,
    partial batch is kept."""
    n = len(spec)
    if not shuffle:
        return (spec[a:a + batch_size] for a in range(0, n, batch_size))
    order = torch.randperm(n).to(spec.device)
    return (spec[order[a:a + batch_size]] for a in range(0, n, batch_size))


def train(dataloader=None, *, n_epochs=1, batch_size=30, lr=0.00002, betas=(0.5, 0.999), display_step=5, save_step=5,
          z_dim=100, model_path="models/", input_hw=None, fake_provider=None, device=None, seed=None,
          compute_dtype=None, elide_dead_backward=False, max_steps=None, save=True, log=print, audio_file=None,
          window_size=5, hop_length_audio=5, shuffle=True, maestro_dir=None, maestro_meta=None):
    """The reference's ``__main__`` training loop (SIMNN.py:234-348) on the fused MI355X step.

    dataloader: iterable of real batches (B,H,W) fp32 (the reference's ``DataLoader(MaestroDataset(batch_size=30),
        batch_size=1, shuffle=True, collate_fn=my_collate)``, both in ``datasets``); if None, seeded synthetic
        spectrogram windows are used (``max_steps`` batches, default 10).
    maestro_dir: a MAESTRO folder to train on instead -- the reference's default configuration, built here:
        ``datasets.MaestroDataset(batch_size, input_folder=maestro_dir, meta_data_file=maestro_meta)``.  Every epoch
        visits the files in a ``torch.randperm`` order (in index order with ``shuffle=False``) and each step trains on
        one file's windows, at most ``batch_size`` of them, as that DataLoader deals them.  The windows are rendered by
        the integer synth that renders the "des" fakes.  ``input_hw`` is (128, 216).
    audio_file: a WAV file to train on instead (``datasets.InputSong(audio_file, window_size, hop_length_audio)``, the
        reference's single-song configuration): every epoch deals the song's windows in batches of ``batch_size``,
        shuffled unless ``shuffle=False``.  ``input_hw`` then defaults to the (128, frames) of the song's windows
        (otherwise to the reference's (128, 216)).
    fake_provider(generated (B,1,20,20) device tensor) -> (B,H,W) tensor: stands in for the DES/FluidSynth bridge
        ``matrix_to_wav`` (SIMNN.py:301); "des": the built-in bridge (``des_fake_provider(0, input_hw[1])``; it needs
        ``input_hw[1] <= 216`` frames, the reference's ``start=0, end=216`` by default); if None, seeded synthetic
        windows are used.  "des_batch": the same bridge with the simulation on the device, one launch per batch
        (``des_fake_provider(0, input_hw[1], batched=True)``; matrix_sim_process lists what differs from "des").  "des_device": the draws on the
        device too, one stream per sample (``batched="des_device"``).
    Returns (gen, disc, gen_losses, disc_losses).
    """
    from .train import SimnnTrainer
    device = torch.device(device if device is not None else "cuda")
    song = maestro = None
    if (audio_file is not None) + (dataloader is not None) + (maestro_dir is not None) > 1:
        raise ValueError("train() takes one of audio_file, dataloader and maestro_dir")
    if maestro_dir is not None:
        from .datasets import MaestroDataset
        if input_hw is not None and tuple(input_hw) != (128, 216):
            raise ValueError(f"input_hw = {tuple(input_hw)} but the windows of a MAESTRO file are (128, 216)")
        input_hw = (128, 216)
        maestro = MaestroDataset(batch_size, input_folder=maestro_dir, meta_data_file=maestro_meta, device=device)
    elif audio_file is not None:
        from .datasets import InputSong
        song = InputSong(audio_file, window_size, hop_length_audio, device=device).spectrograms()
        song_hw = tuple(song.shape[1:])
        if input_hw is not None and tuple(input_hw) != song_hw:
            raise ValueError(f"input_hw = {tuple(input_hw)} but the windows of {audio_file} are {song_hw}")
        input_hw = song_hw
    elif input_hw is None:
        input_hw = (128, 216)
    if isinstance(fake_provider, str):
        msp.check_back_end(fake_provider, "unknown fake_provider", ValueError)
        if input_hw[0] != 128 or not 0 < input_hw[1] <= 216:
            raise ValueError(f"fake_provider=\"{fake_provider}\" makes (128, end - start <= 216) windows, input_hw is "
                             f"{tuple(input_hw)}")
        fake_provider = des_fake_provider(0, input_hw[1], batched=fake_provider)
    if seed is not None:
        torch.manual_seed(seed)
    gen = Generator().to(device)
    disc = Discriminator(input_hw=input_hw).to(device)
    gen = gen.apply(weights_init)
    disc = disc.apply(weights_init)
    trainer = SimnnTrainer(gen, disc, lr=lr, betas=betas, compute_dtype=compute_dtype,
                           elide_dead_backward=elide_dead_backward)
    gen_losses, disc_losses = [], []
    cur_step = 0
    for epoch in range(n_epochs):
        if song is not None:
            batches = _song_batches(song, batch_size, shuffle)
        elif maestro is not None:
            order = torch.randperm(len(maestro)).tolist() if shuffle else range(len(maestro))
            batches = (maestro[i] for i in order)
        elif dataloader is None:
            n = max_steps if max_steps is not None else 10
            batches = (synthetic.spectrogram_batch(batch_size, input_hw, seed=1234 + i) for i in range(n))
        else:
            batches = iter(dataloader)
        for real in batches:
            if max_steps is not None and cur_step >= max_steps:
                break
            real = real.to(device)
            cur_batch_size = len(real)
            noise = get_noise(cur_batch_size, z_dim, device=device)
            if fake_provider is None:
                provider = lambda _adj, n=cur_batch_size, s=cur_step: synthetic.spectrogram_batch(  # noqa: E731
                    n, input_hw, seed=99991 + s)
            else:
                provider = fake_provider
            d_loss, g_loss = trainer.step(real, noise, provider)
            disc_losses.append(d_loss.item())
            gen_losses.append(g_loss.item())
            if cur_step % display_step == 0 and cur_step > 0:
                log(f"Epoch:{epoch} Step {cur_step}: Generator loss: {sum(gen_losses) / len(gen_losses)}, "
                    f"discriminator loss: {sum(disc_losses) / len(disc_losses)}")
            if save and cur_step % save_step == 0 and cur_step > 0:
                os.makedirs(model_path, exist_ok=True)
                torch.save(gen.state_dict(), os.path.join(model_path, f"gen_{cur_step}_{time.time()}.pt"))
            cur_step += 1
    return gen, disc, gen_losses, disc_losses


def main(argv=None):
    """``python -m gan_des_midi_music_gen_amd.SIMNN``: the reference's ``__main__`` training loop, or with
    ``--generate N --checkpoint gen_*.pt --out-dir DIR`` N clips from a trained generator."""
    import argparse
    ap = argparse.ArgumentParser(description="Train model 1 (the reference's SIMNN.py __main__ loop).")
    ap.add_argument("--audio-file", default=None, help="WAV file to train on (default: seeded synthetic windows)")
    ap.add_argument("--maestro-dir", default=None,
                    help="MAESTRO folder (maestro-v3.0.0.json and its MIDI files) to train on, one file per step")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=30)
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--no-save", action="store_true", help="write no generator checkpoints")
    ap.add_argument("--fake-provider", choices=msp.BACK_ENDS, default=None,
                    help="des: fakes from the built-in DES bridge; des_batch: the same with the simulation batched on "
                         "the device; des_device: the draws on the device too (default: seeded synthetic windows)")
    ap.add_argument("--generate", type=int, default=None, metavar="N",
                    help="do not train: write N clips (MIDI + WAV) from --checkpoint into --out-dir (generate_songs)")
    ap.add_argument("--checkpoint", default=None, help="gen_*.pt generator checkpoint for --generate")
    ap.add_argument("--out-dir", default="adj_sim_outputs/songs", help="where --generate writes song_NNNN.mid / .wav")
    ap.add_argument("--max-seconds", type=float, default=None, help="cut the clips of --generate")
    ap.add_argument("--seed", type=int, default=None, help="seed of --generate (torch and numpy)")
    ap.add_argument("--bridge", choices=msp.BACK_ENDS, default="des_batch",
                    help="DES bridge of --generate")
    a = ap.parse_args(argv)
    if a.generate is not None:
        if a.checkpoint is None or a.generate < 1:
            ap.error("--generate N needs N >= 1 and --checkpoint gen_*.pt")
        if a.seed is not None:
            import numpy as np
            torch.manual_seed(a.seed)
            np.random.seed(a.seed)
        songs = generate_songs(a.checkpoint, a.generate, out_dir=a.out_dir, max_seconds=a.max_seconds, bridge=a.bridge)
        for path in (p for pair in zip(songs.midi_paths, songs.wav_paths) for p in pair):
            print(path)
        return
    train(audio_file=a.audio_file, n_epochs=a.epochs, batch_size=a.batch_size, max_steps=a.max_steps,
          save=not a.no_save, fake_provider=a.fake_provider, maestro_dir=a.maestro_dir)


if __name__ == "__main__":
    main()
