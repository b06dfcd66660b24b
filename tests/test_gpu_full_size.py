"""The channel-split K_A (spectrum_real.hip stftRealKernel) at the launch sizes only long renders reach, held to the oracle.

Every other oracle comparison of the channel-split kernels runs a few dozen workgroups; the branches below are taken only when a launch
has many more: the XCD-aware unit remap (real_common.hpp unitOfIndex: >= 64 units) and its uneven last round, the second-generation
delay and the wave priorities of N = 32768 (spectrum_real.hip, LR1 == 4), and the N = 65536 walk's partial last step.  Each case renders
a full-size buffer through a fresh plan and checks the parity chain (tests/parity_chain.py): link 1, mapped pixels within MAP_TOL x the
frame's largest bin of the oracle's, and link 3, RGBA8 (and lines, where asked) byte for byte given the HIP path's own pixels.  Each case
also asserts the launch facts it exists to reach (_launch_facts), so that a change of CU count or plan defaults fails here instead of
quietly dropping coverage.  Frame counts of the cases that are not the bench's own shape are derived from the CU count; the table's
numbers are for 256 CUs and are checked on such a device.

test_full_size_bins_against_fp64 holds the two-for-one split bins (sgz_stage_bins) of three of the cases to the fp64 restatement of
tests/fp64_bins.py, which shares no code with the oracle or the kernels.
"""
import numpy as np
import pytest

from signalizer_amd import api, config, synth

pytestmark = pytest.mark.gpu

BIN_TOL = 4e-6                              # tests/test_gpu_spectrum.py BIN_TOL
PATH_CHANNEL_SPLIT = 8                      # SGZ_PATH_CHANNEL_SPLIT (sgz.h)


def _cus(gpu) -> int:
    import torch
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _launch_facts(plan, frames: int, cus: int, pipelined: bool = False, fetch_window: bool = False) -> dict:
    """What launchStftReal (spectrum_real.hip) and the kernel decide for this plan and frame count, restated on the host."""
    c = plan.cfg
    N = plan.N
    mono = c.channel_mode not in (config.CH_SEPARATE, config.CH_MIDSIDE)
    units = frames * plan.C * (1 if mono else 2)                              # launchStftReal: units
    round_size = cus * {16384: 4, 32768: 2, 65536: 1}[N]                      # api.hip:360 rp.roundSize
    # the window evaluated in the kernel (WCOS): plan.cpp cosWindow (Hann / Hamming, periodic, W == N), api.hip rp.winPhase
    wcos = (c.window_type in (config.WIN_HANN, config.WIN_HAMMING) and c.window_symmetry == config.WIN_PERIODIC
            and c.window_size == N and not fetch_window)
    walk = N == 65536 and not mono and c.channel_mode == config.CH_SEPARATE and wcos and round_size > 0     # spectrum_real.hip:882
    grid = min(units, round_size) if walk else units                                                        # :883
    # unitOfIndex's nb is the launch's size, or for WALK the units a one-unit-per-workgroup launch would have had: units either way
    remap = units >= 64 and round_size >= 8 and round_size % 8 == 0          # real_common.hpp:55
    rounds = -(-units // round_size)
    last_round = units - (rounds - 1) * round_size                            # real_common.hpp:57 nbr of the last round
    extra = last_round & 7                                                    # real_common.hpp:59
    kcus = round_size >> 1                                                    # spectrum_real.hip:189 cus (LR1 == 4 only)
    stagger = N == 32768 and not pipelined and grid >= 2 * kcus               # spectrum_real.hip:198
    prio = N == 32768 and not pipelined and 2 * kcus < grid <= 3 * kcus       # spectrum_real.hip:205
    return dict(units=units, grid=grid, round_size=round_size, remap=remap, rounds=rounds, last_round=last_round, extra=extra,
                stagger=stagger, prio=prio, wcos=wcos, walk=walk, mono=mono,
                walk_steps=units // grid if walk else 1, walk_rem=units % grid if walk else 0)


def _q(cus: int, at256: int) -> int:
    """a frame count of the form 4 m + 1 near at256 * cus / 256 (at256 = 4 m + 1 itself on 256 CUs): 2 (4 m + 1) units end the last
    remap round 2 past a multiple of 8 whenever round sizes are multiples of 8"""
    return 4 * ((at256 - 1) // 4 * cus // 256) + 1


def _cases(cus: int) -> dict:
    """case -> (cfg, frames, input seed (None: the bench's own input), plan options, facts that must hold, facts on 256 CUs)"""
    cfg2 = config.cfg2()
    n32 = dict(window_size=32768, hop=8192)
    return {
        # the bench's launch: 696 workgroups on 2 x CUs slots, a full second generation and a partial third
        "A": (cfg2, 348, None, {}, dict(remap=True, stagger=True, prio=True, mono=False),
              dict(units=696, grid=696, rounds=2, last_round=184, extra=0)),
        "B": (cfg2, _q(cus, 349), 301, {}, dict(remap=True, stagger=True, prio=True, extra=2),
              dict(units=698, grid=698, last_round=186)),
        # a fetched window, three rounds, priorities off (more than three generations), two pairs (pair-major work list)
        "C": (config.spectrum_config(sample_rate=44100.0, window_type=config.WIN_BLACKMAN_HARRIS, num_pairs=2, **n32), 300 * cus // 256,
              302, {}, dict(remap=True, rounds=3, stagger=True, prio=False, wcos=False),
              dict(units=1200, grid=1200, last_round=176, extra=0)),
        # fewer units than one round: the remap's first round is its last, no delay
        "D": (cfg2, _q(cus, 101), 303, {}, dict(remap=True, rounds=1, stagger=False, prio=False, extra=2),
              dict(units=202, grid=202, last_round=202)),
        # Merge: the MONO kernel, one workgroup per (frame, pair)
        "E": (config.spectrum_config(channel_mode=config.CH_MERGE, num_pairs=2, **n32), 348 * cus // 256, 304, {},
              dict(mono=True, remap=True, stagger=True, prio=True), dict(units=696, grid=696, extra=0)),
        # MidSide: the mixed kernel (two workgroups on (l + r) / 2 and (l - r) / 2)
        "F": (config.spectrum_config(channel_mode=config.CH_MIDSIDE, **n32), _q(cus, 349), 305, {},
              dict(mono=False, remap=True, stagger=True, prio=True, extra=2), dict(units=698, grid=698)),
        # the bench's input on a render-queue lane's plan: the delay and the priorities are off
        "G": (cfg2, 348, None, {api.OPT_PIPELINED: 1, api.OPT_FUSED_COLOUR: 16}, dict(remap=True, stagger=False, prio=False),
              dict(units=696, grid=696, extra=0)),
        # N = 16384: four workgroups per CU per round
        "H": (config.spectrum_config(window_size=16384, hop=4096), _q(cus, 701), 306, {}, dict(remap=True, rounds=2, extra=2),
              dict(units=1402, grid=1402, round_size=1024, last_round=378)),
        # N = 65536 WALK: one workgroup per CU walking over the units; the last step is partial and ends an uneven remap round
        "I": (config.cfg5(pairs=5), _q(cus, 349), 307, {}, dict(walk=True, wcos=True, mono=False, remap=True, extra=2),
              dict(units=3490, grid=256, walk_steps=13, walk_rem=162)),
        # N = 65536 MidSide: not a walk, one workgroup per unit
        "J": (config.spectrum_config(sample_rate=96000.0, window_size=65536, hop=16384, channel_mode=config.CH_MIDSIDE, num_pairs=2),
              _q(cus, 201), 308, {}, dict(walk=False, remap=True, extra=4), dict(units=804, grid=804, rounds=4, last_round=36)),
    }


def _setup(gpu, name):
    """(cfg, plan, x, facts) of a case: the plan uploaded with its options, its launch facts asserted"""
    cus = _cus(gpu)
    cfg, frames, seed, opts, want, want256 = _cases(cus)[name]
    W, hop, C = cfg["window_size"], cfg["hop"], cfg["num_pairs"]
    if seed is None:                                                          # bench.py's input
        x = synth.gen(config.CFG2_SEED, 48000, int(config.CFG2_SECONDS * 48000), 2)
    else:
        x = synth.gen(seed, int(cfg["sample_rate"]), W + (frames - 1) * hop, 2 * C)
    plan = api.Plan(cfg)
    for o, v in opts.items():
        plan.set_option(o, v)
    plan.upload()
    assert plan.path & PATH_CHANNEL_SPLIT, plan.path
    assert plan.num_frames(x.shape[1]) == frames
    facts = _launch_facts(plan, frames, cus, pipelined=bool(opts.get(api.OPT_PIPELINED)))
    bad = {k: (facts[k], v) for k, v in want.items() if facts[k] != v}
    if cus == 256:
        bad.update({k: (facts[k], v) for k, v in want256.items() if facts[k] != v})
    assert not bad, ("launch facts (got, want)", bad, facts)
    return cfg, plan, x, facts


def _poison_next(gpu, shape):
    """The next allocation of `shape` float32 comes back full of NaN instead of what the caching allocator last kept there: an output
    entry the launch never writes (a unit the remap skips) is then non-finite, not a stale copy of a right answer.  Returns the poisoned
    block's address: a caller that allocates nothing else before the output can check that the output landed on it."""
    import torch
    torch.cuda.empty_cache()
    t = torch.full(shape, float("nan"), dtype=torch.float32, device=gpu)
    ptr = t.data_ptr()
    del t
    return ptr


def _chain(oracle, plan, cfg, x, gpu, want_lines=False):
    from parity_chain import check_render
    _poison_next(gpu, (plan.num_frames(x.shape[1]), plan.C, plan.sides, plan.P))          # the stage_mapped output check_render asks for
    problems, stats = check_render(oracle, plan, cfg, x, gpu, want_lines=want_lines)
    assert not problems, (problems[:5], stats)
    assert stats["one_sided_nonfinite"] == 0, stats                          # (synth.gen input: every oracle pixel is finite)
    return stats


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "F", "H", "I", "J"])
def test_full_size_launch_against_the_oracle(gpu, oracle, case):
    cfg, plan, x, facts = _setup(gpu, case)
    stats = _chain(oracle, plan, cfg, x, gpu)                                 # image-only: the bench's form (late pixels in K_B)
    print(f"case {case}: {facts}; mapped worst err / max {stats['worst_rel']:.3g}")
    if case == "A":
        stats = _chain(oracle, plan, cfg, x, gpu, want_lines=True)            # lines as well: realLateKernel behind the channel workgroups
        print(f"case A with lines: mapped worst err / max {stats['worst_rel']:.3g}")


def test_full_size_render_queue_against_the_oracle(gpu, oracle):
    """Case G: the bench's input on a plan set up as a render-queue lane (pipelined, 16-pixel fused K_B) through the chain, and the
    queue's own images byte for byte equal to the oracle's colour stage on that plan's mapped pixels"""
    import torch
    cfg, plan, x, facts = _setup(gpu, "G")
    stats = _chain(oracle, plan, cfg, x, gpu)
    print(f"case G: {facts}; mapped worst err / max {stats['worst_rel']:.3g}")
    xg = torch.from_numpy(x).to(gpu)
    want, _ = oracle.decay_colour(oracle.params_from_dict(cfg), plan.stage_mapped(xg).cpu().numpy())
    q = api.RenderQueue(cfg, 3)
    F = plan.num_frames(x.shape[1])
    outs = [torch.zeros((F, plan.P, 4), dtype=torch.uint8, device=gpu) for _ in range(3)]
    torch.cuda.synchronize()
    for o in outs:                                                            # one render on each lane
        q.submit(xg, o)
    q.wait()
    for k, o in enumerate(outs):
        got = o.cpu().numpy()
        assert np.array_equal(got, want), (k, int((got != want).sum()))
    q.close()


@pytest.mark.parametrize("case", ["A", "C", "I"])
def test_full_size_bins_against_fp64(gpu, case):
    """sgz_stage_bins at full size against the fp64 restatement of the two-for-one split (tests/fp64_bins.py): every entry of every frame
    and pair within BIN_TOL x that frame's largest bin, and csf[0], csf[N/2 - 1], csf[N/2], csf[N] -- the signed DC pair, quirk Q3 and the
    entry that needs both channels, settled by whichever channel workgroup finishes second -- each on its own"""
    import torch
    from fp64_bins import separate_bins, window
    cfg, plan, x, facts = _setup(gpu, case)
    N, W, hop, C = plan.N, cfg["window_size"], cfg["hop"], plan.C
    F = plan.num_frames(x.shape[1])
    w = window(cfg["window_type"], cfg["window_symmetry"], W)
    xg = torch.from_numpy(x).to(gpu)
    _poison_next(gpu, (F, C, N + 1))
    bins = plan.stage_bins(xg)                                                # [F][C][N + 1] on the device (case I: 457 MB)
    special = (0, N // 2 - 1, N // 2, N)
    worst, worst_at = 0.0, None
    worst_k = dict.fromkeys(special, 0.0)
    step = 16
    cols = np.arange(W)
    for f0 in range(0, F, step):
        got = bins[f0:f0 + step].cpu().numpy()
        assert np.isfinite(got).all(), f"case {case}: non-finite bins in frames {f0} .. {f0 + got.shape[0] - 1}"
        starts = (f0 + np.arange(got.shape[0]))[:, None] * hop + cols
        for c in range(C):
            ref = separate_bins(x[2 * c][starts], x[2 * c + 1][starts], w, N)
            rel = np.abs(got[:, c] - ref) / np.abs(ref).max(axis=-1, keepdims=True)
            i = np.unravel_index(int(rel.argmax()), rel.shape)
            if rel[i] > worst:
                worst, worst_at = float(rel[i]), (f0 + int(i[0]), c, int(i[1]))
            for k in special:
                worst_k[k] = max(worst_k[k], float(rel[:, k].max()))
    del bins, xg
    msg = f"case {case} ({facts['units']} units): worst err / max {worst:.3g} at (frame, pair, bin) {worst_at}; " \
          f"entries {', '.join(f'csf[{k}] {v:.3g}' for k, v in worst_k.items())}"
    print(msg)
    assert worst <= BIN_TOL, msg
    for k in special:
        assert worst_k[k] <= BIN_TOL, (k, msg)
