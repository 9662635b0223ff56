"""Drop-in surface of model 2 (MMGAN_MIDI_DES/network_tests.py) on MI355X.

    get_noise(n_samples, noise_dim, device='cpu')                                              network_tests.py:43-44
    weights_init(m)                                                                            :47-55
    Generator(z_dim=10, im_chan=1, hidden_dim=64, input_dim=None, adj_size=None, device='cpu') :58-90
    BeatGenerator(z_dim=10, hidden_dim=64, input_dim=None, output_dim=None, device='cpu')      :93-123
    Discriminator(im_chan=1, hidden_dim=16, roll_size=None, device='cpu')                      :126-144
    DiscriminatorCNN(roll_size=(2, 128, 30), hidden_dim=16)                                    :147-160
    MultiModalGAN(z_dim=100, hidden_dim=64, adj_size=(28, 28), roll_size=(2,128,50), input_dim=50, output_dim=16,
                  instrument=None, start=30, end=80, device='cpu')                             :163-206
    TestMultiModalGAN.test_training_loop(batch_size=16) / training_loop(...)                   :208-350
    MultiModalGAN.sample(n) / .generate_midis(n)             (this build: the batched form of generate_midi, :199-206)
    python -m ... --generate N --checkpoint FILE.pth --beats-from FILE.mid                      N files from a checkpoint
    training_loop(..., midi_dir=DIR | pickle_file=FILE) / python -m ... --midi-dir DIR         :229-230 on real data

Module trees and state_dict keys equal the reference's (``gen.{i}.0`` = Linear, ``gen.{i}.1`` = BatchNorm1d,
``conv1/conv2/fc``), so the committed ``mmgan_64_64_epoch_*.pth`` files load with ``strict=True``.  The nn children
are parameter containers only; every forward runs through the HIP kernels of include/gdm.h.

The DES bridge ``matrix_to_midi`` (network_tests.py:189) is opt-in: ``MultiModalGAN`` takes ``fake_provider="des"`` (or
"des_batch": the simulation batched on the device, matrix_to_midi(simulate="des_batch")) for
the built-in bridge (matrix_sim_process.matrix_to_midi(simulate="des"): DES core + one batched log -> MIDI -> piano-roll
launch) or an injected ``fake_provider(gen_output1, gen_output2, count) -> (rolls (B,2,128,T) tensor,
failed_sim_count)``; without one, forward raises.
"""
import os
import pickle
import time
import unittest

import torch
from torch import nn

from . import functional as Fn
from . import synthetic
from .matrix_sim_process import BACK_ENDS, check_back_end, matrix_to_midi, matrix_to_midis


def get_noise(n_samples, noise_dim, device="cpu"):
    return torch.randn(n_samples, noise_dim, device=device)


def weights_init(m):
    if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
        nn.init.normal_(m.weight, mean=0, std=1)
    if isinstance(m, nn.BatchNorm2d):
        nn.init.xavier_normal_(m.weight)
        nn.init.constant_(m.bias, 0.0)
    if isinstance(m, nn.Linear):
        nn.init.xavier_normal_(m.weight)
        nn.init.constant_(m.bias, 0.0)


def _dtype_of(module):
    cd = getattr(module, "compute_dtype", None)
    return Fn.get_compute_dtype() if cd is None else Fn._NAMES[cd]


def _gen_stack(dims):
    return nn.Sequential(*[nn.Sequential(nn.Linear(i, o), nn.BatchNorm1d(o), nn.Sigmoid())
                           for i, o in zip(dims[:-1], dims[1:])])


def _run_gen_stack(module, x):
    flat, buffers = [], []
    for blk in module.gen:
        lin, bn = blk[0], blk[1]
        flat += [lin.weight, lin.bias, bn.weight, bn.bias]
        buffers.append((bn.running_mean, bn.running_var, bn.num_batches_tracked))
    return Fn.MlpBnSigmoidFn.apply(x, *flat, tuple(buffers), module.training, _dtype_of(module))


def _eval_layers(module):
    return [(blk[0].weight.detach(), blk[0].bias.detach(), blk[1].weight.detach(), blk[1].bias.detach(),
             blk[1].running_mean, blk[1].running_var) for blk in module.gen]


def _eval_geometry(module):
    """(K1, H1, H2, H3, N4) if the one-launch eval kernel takes this generator, else None."""
    from . import ops
    if len(module.gen) != 4 or len({blk[1].eps for blk in module.gen}) != 1:
        return None
    dims = (module.gen[0][0].in_features, *[blk[0].out_features for blk in module.gen])
    return dims if ops.mmgan_gen_eval_supported(*dims) else None


def _eval_pack(module):
    """The generator's weight pack for ops.mmgan_gen_eval, rebuilt when a parameter or a running statistic changed
    (keyed on their data_ptr and _version, as model 1's _eval_cache).  The pack is a copy: it aliases no parameter."""
    from . import ops
    layers = _eval_layers(module)
    ver = tuple(v for la in layers for t in la for v in (t.data_ptr(), t._version))
    hit = module._eval_cache.get("pack")
    if hit is not None and hit[0] == ver and hit[1].device == layers[0][0].device:
        return hit[1], hit[2]
    pack, dims = ops.mmgan_gen_eval_pack(layers, eps=module.gen[0][1].eps)
    module._eval_cache["pack"] = (ver, pack, dims)
    return pack, dims


class Generator(nn.Module):
    """cat(noise, input_tensor) -> 4 x [Linear, BatchNorm1d, Sigmoid] -> (B, im_chan, adj0, adj1) DES matrix."""

    def __init__(self, z_dim=10, im_chan=1, hidden_dim=64, input_dim=None, adj_size=None, device="cpu"):
        super().__init__()
        self.z_dim = z_dim
        self.adj_size = adj_size
        self.device = device
        if input_dim is None:
            input_dim = z_dim
        self.input_tensor_dim = input_dim
        self.gen = _gen_stack([z_dim + input_dim, hidden_dim * 4, hidden_dim * 2, hidden_dim,
                               im_chan * adj_size[0] * adj_size[1]])
        self.gen.apply(weights_init)
        self.compute_dtype = None
        self._eval_cache = {}      # the one-launch eval kernel's weight pack (MultiModalGAN.sample), not module state

    def make_gen_block(self, input_dim, output_dim):
        return nn.Sequential(nn.Linear(input_dim, output_dim), nn.BatchNorm1d(output_dim), nn.Sigmoid())

    def forward(self, noise, input_tensor=None):
        if input_tensor is None:
            input_tensor = torch.randn(len(noise), self.input_tensor_dim).to(noise.device)   # CPU RNG, as the reference
        x = torch.cat((noise, input_tensor.to(noise.device)), dim=1)
        out = _run_gen_stack(self, x)
        return out.view(len(noise), -1, self.adj_size[0], self.adj_size[1])


class BeatGenerator(nn.Module):
    """cat(noise, beats) -> 4 x [Linear, BatchNorm1d, Sigmoid] -> (B, output_dim) DES/MIDI parameters."""

    def __init__(self, z_dim=10, hidden_dim=64, input_dim=None, output_dim=None, device="cpu"):
        super().__init__()
        self.z_dim = z_dim
        self.output_dim = output_dim
        if input_dim is None:
            input_dim = z_dim
        self.input_tensor_dim = input_dim
        self.device = device
        self.gen = _gen_stack([z_dim + input_dim, hidden_dim * 4, hidden_dim * 2, hidden_dim, output_dim])
        self.gen.apply(weights_init)
        self.compute_dtype = None
        self._eval_cache = {}      # the one-launch eval kernel's weight pack (MultiModalGAN.sample), not module state

    def make_gen_block(self, input_dim, output_dim):
        return nn.Sequential(nn.Linear(input_dim, output_dim), nn.BatchNorm1d(output_dim), nn.Sigmoid())

    def forward(self, noise, input_tensor=None):
        if input_tensor is None:
            input_tensor = torch.randn(len(noise), self.input_tensor_dim).to(noise.device)
        x = torch.cat((noise, input_tensor.to(noise.device)), dim=1)
        return _run_gen_stack(self, x)


class Discriminator(nn.Module):
    """MLP discriminator: 3 x [Linear, LeakyReLU(0.2)] (the last LeakyReLU acts on the logit, as in the reference)."""

    def __init__(self, im_chan=1, hidden_dim=16, roll_size=None, device="cpu"):
        super().__init__()
        self.roll_size = roll_size
        self.device = device
        dims = [im_chan * roll_size[0] * roll_size[1] * roll_size[2], hidden_dim, hidden_dim * 2, 1]
        self.disc = nn.Sequential(*[nn.Sequential(nn.Linear(i, o), nn.LeakyReLU(0.2, inplace=True))
                                    for i, o in zip(dims[:-1], dims[1:])])
        self.compute_dtype = None

    def make_disc_block(self, input_dim, output_dim):
        return nn.Sequential(nn.Linear(input_dim, output_dim), nn.LeakyReLU(0.2, inplace=True))

    def forward(self, image):
        flat = []
        for blk in self.disc:
            flat += [blk[0].weight, blk[0].bias]
        return Fn.MlpLeakyFn.apply(image, *flat, _dtype_of(self))


class DiscriminatorCNN(nn.Module):
    """(B,2,128,T) piano-roll -> logits (B,1): Conv(k4,s2,p1) LeakyReLU, Conv(k4,s2,p1) LeakyReLU, flatten, Linear."""

    def __init__(self, roll_size=(2, 128, 30), hidden_dim=16):
        super().__init__()
        self.conv1 = nn.Conv2d(roll_size[0], hidden_dim, kernel_size=4, stride=2, padding=1)
        self.conv2 = nn.Conv2d(hidden_dim, hidden_dim * 2, kernel_size=4, stride=2, padding=1)
        self.leaky_relu = nn.LeakyReLU(0.2, inplace=True)
        self.final_size = hidden_dim * 2 * ((roll_size[1] // 4) * (roll_size[2] // 4))
        self.fc = nn.Linear(self.final_size, 1)
        self.compute_dtype = None

    def forward(self, image):
        return Fn.DcnnFn.apply(image, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                               self.fc.weight, self.fc.bias, _dtype_of(self))


def _no_bridge(*_a, **_k):
    raise RuntimeError("MultiModalGAN needs a fake_provider: the DES/MIDI bridge (matrix_to_midi, "
                       "MMGAN_MIDI_DES/network_tests.py:189) is outside the scope of this build; pass "
                       "fake_provider=callable(gen_output1, gen_output2, count) -> (rolls, failed_sim_count)")


def des_fake_provider(adj_size, instrument, start, end, generate=False, midi_path=None, batched=False):
    """The built-in bridge as a fake_provider: the reference's matrix_to_midi call (network_tests.py:189 / :204) with
    the DES core and the batched log -> MIDI -> piano-roll kernel behind it; the rolls stay on the device.
    batched: simulate all samples in one device launch (matrix_to_midi(simulate="des_batch")); a back end's name
    ("des_batch", "des_device") selects that one."""
    simulate = batched if isinstance(batched, str) else ("des_batch" if batched else "des")

    def provider(gen_output1, gen_output2, count):
        return matrix_to_midi(gen_output1, gen_output2, adj_size=adj_size, instrument=instrument, start=start, end=end,
                              count=0 if count is None else count, generate=generate, simulate=simulate,
                              return_tensor=True, midi_path=midi_path)
    return provider


class MultiModalGAN(nn.Module):
    def __init__(self, z_dim=100, hidden_dim=64, adj_size=(28, 28), roll_size=(2, 128, 50), input_dim=50,
                 output_dim=16, instrument=None, start=30, end=80, device="cpu", fake_provider=None, midi_path=None):
        super().__init__()
        self.z_dim = z_dim
        self.generator1 = Generator(z_dim, hidden_dim=hidden_dim, adj_size=adj_size, device=device).to(device)
        self.generator2 = BeatGenerator(z_dim, hidden_dim=hidden_dim, input_dim=input_dim, output_dim=output_dim,
                                        device=device).to(device)
        self.discriminator = DiscriminatorCNN(roll_size=roll_size).to(device)
        self.instrument = instrument
        self.start = start
        self.end = end
        self.adj_size = adj_size
        self.device = device
        self.midi_path = midi_path          # where generate_midi's built-in bridge writes (default: upstream's path)
        self.generate_provider = None
        if isinstance(fake_provider, str):
            check_back_end(fake_provider, "unknown fake_provider", ValueError)
            batched = fake_provider
            fake_provider = des_fake_provider(adj_size, instrument, start, end, batched=batched)
            self.generate_provider = des_fake_provider(adj_size, instrument, start, end, generate=True,
                                                       midi_path=midi_path, batched=batched)
        self.fake_provider = fake_provider if fake_provider is not None else _no_bridge

    def forward(self, noise1, noise2, input_tensor, count, make_dot_png=True):
        gen_output1 = self.generator1(noise1)
        gen_output2 = self.generator2(noise2, input_tensor)
        # make_dot_png: the reference renders a torchviz graph here (network_tests.py:180-188); torchviz/graphviz
        # are not part of this build, the flag is accepted and ignored.
        sim_output, failed_sim_count = self.fake_provider(gen_output1.detach(), gen_output2.detach(), count)
        if not torch.is_tensor(sim_output):   # list of per-sample numpy rolls, like matrix_to_midi returns
            sim_output = torch.stack([torch.as_tensor(s).float() for s in sim_output])
        sim_output = sim_output.to(noise1.device)
        return self.discriminator(sim_output), failed_sim_count

    def generate_midi(self, noise1, noise2, input_tensor):
        self.generator1.eval()
        self.generator2.eval()
        with torch.no_grad():
            gen_output1 = self.generator1(noise1)
            gen_output2 = self.generator2(noise2, input_tensor)
        provider = self.generate_provider if self.generate_provider is not None else self.fake_provider
        sim_output, _failed = provider(gen_output1.detach(), gen_output2.detach(), None)
        return sim_output


    def sample(self, n_samples=None, *, noise1=None, noise2=None, input_tensor=None, gen1_input=None,
               compute_dtype="bf16"):
        """Draw n generator outputs in eval arithmetic: (gen_output1 (n,1,adj0,adj1), gen_output2 (n,output_dim)), fp32
        and contiguous on the module's device -- what ``matrix_to_midi`` / ``matrix_to_midis`` read in place.

        Noise that is not given is drawn with ``get_noise`` on the device (noise1, then noise2); generator 1's second
        input half (``gen1_input``) and a missing ``input_tensor`` are then drawn as the generators' ``forward`` draws
        them: ``torch.randn`` on the CPU, then moved.  input_tensor (the beats) is (n, input_dim) or (1, input_dim):
        one vector for every sample, broadcast inside the kernel.  BatchNorm runs on its running statistics whatever
        ``.training`` says and no state of the module changes: parameters, running statistics,
        ``num_batches_tracked``, ``training`` and ``compute_dtype`` are as before.
        compute_dtype "bf16" (default): both generators in ONE launch for any n (ops.mmgan_gen_eval); "fp32", or a
        geometry the kernel does not take, walks the module forwards in eval mode (and restores ``training``)."""
        from . import ops
        g1, g2 = self.generator1, self.generator2
        dev = g1.gen[0][0].weight.device
        given = [t.shape[0] for t in (noise1, noise2, gen1_input) if t is not None]
        if input_tensor is not None and input_tensor.shape[0] != 1:
            given.append(input_tensor.shape[0])
        n = int(n_samples) if n_samples is not None else (max(given) if given else None)
        if n is None:
            raise ValueError("sample needs n_samples or a noise tensor")
        if n < 1 or any(k != n for k in given):
            raise ValueError(f"sample: n_samples = {n} but the given tensors hold {given} rows")
        noise1 = get_noise(n, g1.z_dim, device=dev) if noise1 is None else noise1.to(dev)
        noise2 = get_noise(n, g2.z_dim, device=dev) if noise2 is None else noise2.to(dev)
        gen1_input = (torch.randn(n, g1.input_tensor_dim) if gen1_input is None else gen1_input).to(dev)
        input_tensor = (torch.randn(n, g2.input_tensor_dim) if input_tensor is None else input_tensor).to(dev)
        geo = (_eval_geometry(g1), _eval_geometry(g2))
        if Fn._NAMES[compute_dtype] == Fn.BF16 and None not in geo and geo[0][1:4] == geo[1][1:4]:
            jobs = []
            for g, noise, inp in ((g1, noise1, gen1_input), (g2, noise2, input_tensor)):
                pack, dims = _eval_pack(g)
                jobs.append(dict(noise=noise.float().contiguous(), input=inp.float().contiguous(), pack=pack, dims=dims))
            out1, out2 = ops.mmgan_gen_eval(jobs)
            return out1.view(n, -1, self.adj_size[0], self.adj_size[1]), out2
        was = [(g.training, g.compute_dtype) for g in (g1, g2)]
        try:
            for g in (g1, g2):
                g.eval()
                g.compute_dtype = compute_dtype
            with torch.no_grad():
                out1 = g1(noise1, gen1_input)
                out2 = g2(noise2, input_tensor.expand(n, -1))
        finally:
            for g, (training, cd) in zip((g1, g2), was):
                g.train(training)
                g.compute_dtype = cd
        return out1.detach().contiguous(), out2.detach().contiguous()

    def generate_midis(self, n_samples=None, *, noise1=None, noise2=None, input_tensor=None,
                       out_dir="adj_sim_outputs/midi", name="generation_{:04d}.mid", bridge="des_batch",
                       compute_dtype="bf16"):
        """``generate_midi`` for a batch that keeps every sample: ``sample`` (one launch), then
        ``matrix_sim_process.matrix_to_midis`` with the module's adj_size, instrument, start and end, which writes
        ``out_dir/name.format(i)`` for every sample whose simulation and MIDI conversion succeeded.  Works whatever
        ``fake_provider`` the module was built with: bridge names the built-in one, "des", "des_batch" or
        "des_device".
        Returns the MidiBatch (rolls, tracks, ok, reasons) with ``paths``: None where ``ok`` is false."""
        out1, out2 = self.sample(n_samples, noise1=noise1, noise2=noise2, input_tensor=input_tensor,
                                 compute_dtype=compute_dtype)
        paths = [os.path.join(out_dir, name.format(i)) for i in range(out1.shape[0])]
        return matrix_to_midis(out1, out2, self.adj_size, self.instrument, self.start, self.end, simulate=bridge,
                               midi_paths=paths)


def training_loop(batch_size=16, *, num_epochs=100, train_loader=None, steps_per_epoch=None, fake_provider=None,
                  device=None, noise_dim=50, gen2_output_dim=20, max_beat_length=50, adj_size=(64, 64),
                  sequence_length=50, lr=0.01, model_path=None, save_dir=None, compute_dtype=None,
                  elide_dead_backward=False, print_interval=10, seed=None, epoch_sleep=0.0, log=print,
                  criterion="bce", midi_dir=None, pickle_file=None, sample_size=300):
    """The body of ``TestMultiModalGAN.test_training_loop`` (network_tests.py:209-350) on the fused MI355X step.

    train_loader: iterable of (piano_roll, durations, beats) batches (the reference's MaestroDatasetPickle loader,
        batch_size, drop_last); None -> seeded MAESTRO-shaped synthetic batches (``steps_per_epoch``, default 8).
    midi_dir: a directory (or list) of MIDI files -> ``datasets.MaestroWindows.from_midi(midi_dir, sample_size,
        sequence_length, max_beat_length)``, the dataset notebook cell 11 pickles, built once on the device;
        pickle_file: path of such a pickle (``preprocessed_data_{sequence_length}.pkl``) -> ``MaestroDatasetPickle``.
        Either feeds every epoch with ``batches(batch_size)``: unshuffled, drop_last, as the reference's DataLoader
        (network_tests.py:229-230).  At most one of train_loader / midi_dir / pickle_file.
    fake_provider(g1_out, g2_out, count) -> ((B,2,128,T) tensor, failed): the DES bridge; "des" -> the built-in one
        (DES core + batched log -> MIDI -> piano-roll kernel); "des_batch" -> the same with the simulation batched on
        the device (matrix_sim_process lists what differs); "des_device" -> the draws on the device too, one stream
        per sample; None -> synthetic rolls.
    save_dir: if given, per-epoch ``losses/*.pkl`` and ``models/mmgan_{a}_{b}_epoch_{e}.pth`` are written there with
        the reference's file names; model_path: state_dict to resume from (optimizer state is not saved, as upstream).
    criterion: "bce" | "mse" | "l1" -- the reference picks one by moving a comment (network_tests.py:248-250:
        nn.BCEWithLogitsLoss(), nn.MSELoss(), nn.L1Loss()).
    Returns (disc_losses, gen_losses) of the last epoch, like the reference.
    """
    if sum(src is not None for src in (train_loader, midi_dir, pickle_file)) > 1:
        raise ValueError("give at most one of train_loader, midi_dir and pickle_file")
    from .train import MmganTrainer, StepLR
    device = torch.device(device if device is not None else "cuda")
    if midi_dir is not None or pickle_file is not None:
        from . import datasets
        if midi_dir is not None:
            dataset = datasets.MaestroWindows.from_midi(midi_dir, sample_size, sequence_length, max_beat_length, device)
        else:
            dataset = datasets.MaestroDatasetPickle(pickle_file, sequence_length, max_beat_length, device, data_dir="")
        if tuple(dataset.piano_roll.shape[1:]) != (128, sequence_length):
            raise ValueError(f"the dataset's rolls are {tuple(dataset.piano_roll.shape[1:])}, the model takes "
                             f"(128, {sequence_length})")
        if len(dataset) < batch_size:
            raise ValueError(f"the dataset holds {len(dataset)} windows, fewer than one batch of {batch_size}")
        train_loader = dataset.batches(batch_size)
    if seed is not None:
        torch.manual_seed(seed)
    roll_size = (2, 128, sequence_length)
    start = 100
    if isinstance(fake_provider, str):
        check_back_end(fake_provider, "unknown fake_provider", ValueError)
        fake_provider = des_fake_provider(adj_size, 0, start, start + sequence_length, batched=fake_provider)
    mmgan = MultiModalGAN(z_dim=noise_dim, adj_size=adj_size, roll_size=roll_size, input_dim=max_beat_length,
                          output_dim=gen2_output_dim, instrument=0, start=start, end=start + sequence_length,
                          device=device, fake_provider=fake_provider)
    if model_path is not None and os.path.isfile(model_path):
        mmgan.load_state_dict(torch.load(model_path, map_location=device, weights_only=True))
        log(f"Loaded model from {model_path}")
    trainer = MmganTrainer(mmgan, lr=lr, compute_dtype=compute_dtype, elide_dead_backward=elide_dead_backward,
                           criterion=criterion)
    disc_scheduler = StepLR(trainer, step_size=30, gamma=0.1)   # the generator optimizer never has gradients
    count = total_failures = total_seen = 0
    disc_losses, gen_losses = [], []
    for epoch in range(num_epochs):
        mmgan.train()
        disc_losses, gen_losses = [], []
        if train_loader is None:
            n = steps_per_epoch if steps_per_epoch is not None else 8
            loader = ((d["piano_roll"], d["durations"], d["beats"]) for d in
                      (synthetic.mmgan_inputs(batch_size, sequence_length, seed=1234 + epoch * 100003 + i)
                       for i in range(n)))
        else:
            loader = iter(train_loader)
        for i, (piano_roll, durations, beats) in enumerate(loader):
            if steps_per_epoch is not None and i >= steps_per_epoch:
                break
            count += 1
            piano_roll, durations, beats = piano_roll.to(device), durations.to(device), beats.to(device)
            noise1 = torch.randn(batch_size, noise_dim, device=device)
            noise2 = torch.randn(batch_size, noise_dim, device=device)
            failed = [0]

            def bridge(g1, g2, _count=count, _i=i):
                if fake_provider is None:
                    d = synthetic.mmgan_inputs(batch_size, sequence_length, seed=777 + _count * 2 + len(failed))
                    failed.append(0)
                    return d["fake_a"].to(device)
                rolls, nfail = fake_provider(g1, g2, _count)
                failed.append(nfail)
                if not torch.is_tensor(rolls):
                    rolls = torch.stack([torch.as_tensor(r).float() for r in rolls])
                return rolls.to(device)

            d_loss, g_loss = trainer.step(piano_roll, durations, beats, noise1, noise2, bridge, bridge)
            total_failures += failed[-1]
            total_seen += batch_size
            disc_losses.append(d_loss.item())
            gen_losses.append(g_loss.item())
            if i % 5 == 0:
                log(f"Epoch {epoch + 1}/{num_epochs}, Batch {i}, Avg Disc Loss: {sum(disc_losses) / len(disc_losses)}, "
                    f"Avg Gen Loss: {sum(gen_losses) / len(gen_losses)}")
                log(f"Total failures: {total_failures} Total seen: {total_seen}")
        disc_scheduler.step()
        if save_dir is not None:
            os.makedirs(os.path.join(save_dir, "losses"), exist_ok=True)
            os.makedirs(os.path.join(save_dir, "models"), exist_ok=True)
            with open(os.path.join(save_dir, "losses", f"disc_losses_epoch_{epoch + 1}.pkl"), "wb") as f:
                pickle.dump(disc_losses, f)
            with open(os.path.join(save_dir, "losses", f"gen_losses_epoch_{epoch + 1}.pkl"), "wb") as f:
                pickle.dump(gen_losses, f)
            torch.save(mmgan.state_dict(), os.path.join(
                save_dir, "models", f"mmgan_{adj_size[0]}_{adj_size[1]}_epoch_{epoch + 1}.pth"))
        if (epoch + 1) % print_interval == 0 and disc_losses:
            log(f"Epoch {epoch + 1}/{num_epochs}, Avg Disc Loss: {sum(disc_losses) / len(disc_losses)}, "
                f"Avg Gen Loss: {sum(gen_losses) / len(gen_losses)}")
        if epoch_sleep:
            time.sleep(epoch_sleep)   # the reference sleeps 10 s per epoch (network_tests.py:344); off by default
    return disc_losses, gen_losses


class TestMultiModalGAN(unittest.TestCase):
    def test_training_loop(self, batch_size=16):
        """Same entry point as the reference's unittest; runs a short synthetic-data schedule (no MAESTRO file ships
        with this build: ``training_loop(midi_dir=...)`` / ``pickle_file=...`` is the real-data route)."""
        if not torch.cuda.is_available():
            self.skipTest("needs a HIP device")
        # network_tests.py:211: the reference's loop runs under anomaly detection; here that makes every iteration check
        # its inputs, losses and discriminator state for NaN / Inf (train._TrainerBase.check_finite).  The reference
        # leaves the flag set; this entry point restores what it found.
        was = torch.is_anomaly_enabled()
        torch.autograd.set_detect_anomaly(True)
        try:
            return training_loop(batch_size, num_epochs=1, steps_per_epoch=4, log=lambda *_a: None)
        finally:
            torch.autograd.set_detect_anomaly(was)


_CLI_OPTIONS = ("--midi-dir", "--pickle", "--epochs", "--batch-size", "--sequence-length", "--sample-size",
                "--fake-provider", "--save-dir", "--max-steps")


def generate_main(argv):
    """``--generate N --checkpoint FILE.pth --beats-from FILE.mid``: N MIDI files from a trained model 2, as the
    reference's demo notebook makes one (mmgan.generate_midi(noise, noise, get_beats()[:50])): the checkpoint is loaded
    ``strict=True`` into the 64x64 geometry of the committed mmgan_64_64_epoch_*.pth files, the beats are the first 50
    of the file's beat grid (zero-padded), one line is printed per written file."""
    import argparse
    import numpy as np
    from . import datasets
    ap = argparse.ArgumentParser(prog="gan_des_midi_music_gen_amd.network_tests --generate", description=generate_main.__doc__)
    ap.add_argument("--generate", type=int, required=True, metavar="N")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--beats-from", required=True, metavar="FILE.mid")
    ap.add_argument("--out-dir", default="adj_sim_outputs/midi")
    ap.add_argument("--instrument", type=int, default=0)
    ap.add_argument("--start", type=int, default=100)
    ap.add_argument("--end", type=int, default=150)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--bridge", choices=BACK_ENDS, default="des_batch")
    a = ap.parse_args(argv)
    if a.generate < 1:
        ap.error("--generate needs N >= 1")
    device = torch.device("cuda")
    if a.seed is not None:
        torch.manual_seed(a.seed)
        np.random.seed(a.seed)
    mmgan = MultiModalGAN(z_dim=50, adj_size=(64, 64), roll_size=(2, 128, 50), input_dim=50, output_dim=20,
                          instrument=a.instrument, start=a.start, end=a.end, device=device)
    mmgan.load_state_dict(torch.load(a.checkpoint, map_location=device, weights_only=True), strict=True)
    beats = datasets._fit_beats(datasets.get_beats(datasets.read_midi(a.beats_from)), 50)
    res = mmgan.generate_midis(a.generate, input_tensor=torch.as_tensor(np.asarray(beats), dtype=torch.float32)[None],
                               out_dir=a.out_dir, bridge=a.bridge)
    for i, path in enumerate(res.paths):
        print(path if path is not None else f"sample {i}: no file ({res.reasons[i]})")
    return 0


def main(argv=None):
    """``python -m gan_des_midi_music_gen_amd.network_tests``: with --generate, ``generate_main``; with --midi-dir or
    --pickle, ``training_loop`` on that data; without any of the options below, the reference's ``unittest.main()``."""
    import argparse
    import sys
    argv = sys.argv[1:] if argv is None else list(argv)
    if any(a.split("=")[0] == "--generate" for a in argv):
        return generate_main(argv)
    if not any(a.split("=")[0] in _CLI_OPTIONS for a in argv):
        return unittest.main(argv=[sys.argv[0]] + argv)
    ap = argparse.ArgumentParser(prog="gan_des_midi_music_gen_amd.network_tests", description=main.__doc__)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--midi-dir", help="directory of MIDI files (MaestroWindows.from_midi)")
    src.add_argument("--pickle", help="preprocessed_data_{L}.pkl of notebook cell 11 (MaestroDatasetPickle)")
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--sequence-length", type=int, default=50)
    ap.add_argument("--sample-size", type=int, default=300)
    ap.add_argument("--fake-provider", choices=BACK_ENDS, default=None,
                    help="des: the built-in DES bridge; des_batch: the same with the simulation batched on the "
                         "device; des_device: the draws on the device too; default: synthetic fake rolls")
    ap.add_argument("--save-dir", default=None)
    ap.add_argument("--max-steps", type=int, default=None, help="steps per epoch at most")
    a = ap.parse_args(argv)
    training_loop(a.batch_size, num_epochs=a.epochs, midi_dir=a.midi_dir, pickle_file=a.pickle,
                  sample_size=a.sample_size, sequence_length=a.sequence_length, fake_provider=a.fake_provider,
                  save_dir=a.save_dir, steps_per_epoch=a.max_steps)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
