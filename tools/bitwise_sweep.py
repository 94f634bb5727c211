"""Compares the outputs of two builds of the library bitwise (diagnostics: every launch plan and fused kernel must produce the
same bits).  One child process per library -- this tree's release build, then the other -- and SHA-256 of what each returns.

usage: python tools/bitwise_sweep.py <other libiris_hifigan_*.so> [f32|bf16] [n_random_shapes]
       python tools/bitwise_sweep.py <other libiris_hifigan_*.so> dsp [out.json]

f32 / bf16: the vocoder's waveforms over 63 (batch, frames) shapes.
dsp: the DSP stages on the small shapes of their own case tables (oracle/dsp_chain_cases.py, tests/denoiser_cases.py) --
MelFrontend dense and ragged, fp32 and int16; GriffinLim dense and ragged at n_iter 0, 1 and 2, with a host phase and with the
device-drawn one; Denoiser.forward_device at strength 1 and 0.3, dense and with ragged lengths (full, 0, 1, inside a block, on
a block edge); estimate_bias; a DenoiserSession fed each case in three uneven pushes.  out.json gets the counts and hashes."""
import os, subprocess, sys, json
from pathlib import Path
import numpy as np
REPO = Path(__file__).resolve().parents[1]
shapes = [(1, t) for t in (1, 2, 3, 5, 7, 13, 31, 40, 50, 63, 64, 65, 77, 99, 100, 117, 118, 119, 127, 128, 129, 150, 199, 230, 257, 282, 301, 333, 390, 391, 450)] + \
         [(2, 50), (2, 117), (3, 33), (3, 100), (4, 64), (5, 21), (7, 13), (8, 40), (12, 40), (16, 9), (2, 282), (3, 200), (1, 700), (1, 1000), (4, 500)] + \
         [(1, t) for t in (350, 400, 500, 550, 600, 650, 750, 800, 850, 900, 950, 1100, 1400, 1600)] + [(2, 700), (3, 500), (4, 400)] + \
         [(32, 500), (8, 300), (9, 130), (24, 57)]   # snake-ordered job plans; batches whose tiles qualify for XCD grouping only together
mode = sys.argv[2] if len(sys.argv) > 2 else "f32"
if mode != "dsp" and len(sys.argv) > 3:          # optional third argument: that many extra random shapes (seeded): 1 <= B <= 5, 1 <= T <= 1600
    rng = np.random.default_rng(20260)
    shapes = shapes + [(int(rng.integers(1, 6)), int(rng.integers(1, 1601))) for _ in range(int(sys.argv[3]))]
code = r'''
import sys, json, hashlib, torch
sys.path.insert(0, "iris-tts_amd")
from iris._engine import GeneratorEngine
from iris._weights import GeneratorConfig, seeded_mel, seeded_state_dict
shapes = json.loads(sys.argv[1]); dtype = sys.argv[2]
cfg = GeneratorConfig(); eng = GeneratorEngine(cfg, seeded_state_dict(cfg, seed=11, gain=1.15, post_gain=12.0), torch.device("cuda", 0))
out = {}
for B, T in shapes:
    y = eng.forward(torch.from_numpy(seeded_mel(100 + T, B, T)).cuda(), dtype=dtype)
    out[f"{B}x{T}"] = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()
print(json.dumps(out))
'''
dsp_code = r'''
import sys, json, hashlib
import numpy as np, torch
repo = sys.argv[1]
sys.path[:0] = [repo + "/iris-tts_amd", repo, repo + "/tests"]
from oracle import dsp_chain_cases as D
import denoiser_cases as C
from iris.mel import MelFrontend
from iris.griffin_lim import pack_phase
from iris.denoiser import Denoiser
dev = torch.device("cuda", 0)
out = {}
def put(key, *tensors):
    assert key not in out, key
    out[key] = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in tensors)).hexdigest()
def on(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

fe = {name: MelFrontend(**cfg) for name, cfg in D.MEL_CONFIGS.items()}
for name, B, L in D.MEL_CASES:
    for seed in D.MEL_SEEDS:
        a = D.mel_audio(name, B, L, seed)
        for tag, x in (("f32", a), ("i16", D.to_int16(a))):
            put(f"mel/{name}-B{B}-L{L}/seed{seed}/{tag}", *fe[name].forward_device(x))
for name, L, ns in D.MEL_RAGGED:
    a = D.mel_audio(name, len(ns), L, 3)
    for tag, x in (("f32", a), ("i16", D.to_int16(a))):
        for caps in (None, [10 ** 6, 10 ** 6, 0, 9, 10 ** 6]):
            put(f"mel_ragged/{name}-L{L}/caps{caps is not None}/{tag}", *fe[name].forward_device(x, lengths=list(ns), max_frames=caps))

gl_runs = [(D.case_id(c), c, None) for c in D.GL_CASES] + [(f"{n}-T{T}-ragged", (n, len(ls), T), ls) for n, T, ls in D.GL_RAGGED]
for cid, case, lengths in gl_runs:
    lm, packed = D.gl_logmel(case), on(pack_phase(D.gl_phase(case, D.GL_SEEDS[0])))
    kw = {} if lengths is None else {"lengths": torch.tensor(lengths, dtype=torch.int32, device=dev)}
    for n_iter in (0, 1, 2):
        gl = D.gl_model(case[0], n_iter=n_iter)
        put(f"gl/{cid}/n_iter{n_iter}/host_phase", gl.forward_device(lm, packed, **kw))
        put(f"gl/{cid}/n_iter{n_iter}/device_phase", gl.forward_device(lm, "device", seed=99, first_item=3, **kw))

for case in C.CASES:
    name, B, M = case
    cfg, cid = C.CONFIGS[name], C.case_id(case)
    n_fft, hop, win = C.stft_args(name)
    dn = Denoiser(n_fft, hop, win, strength=C.STRENGTH, bias=C.bias(case), device=dev)
    wav = on(C.waveform(case))
    five = on(np.stack([C.waveform_item(hop * M, cfg, seed=b) for b in range(5)]))
    ragged = [M, 0, 1, max(M // 2, 1), min(M, 31)]            # T_b = M_b + 1: full, none, none (one frame), inside a block, 32 frames
    cuts = (M // 5, M // 5 + M // 2)                           # three uneven pushes
    for strength in (1.0, 0.3):
        put(f"dn/{cid}/strength{strength}/dense", dn.forward_device(wav, strength=strength))
        put(f"dn/{cid}/strength{strength}/ragged", dn.forward_device(five, lengths=ragged, strength=strength))
        s = dn.open_session(strength=strength)
        pieces = [s.push(wav[:, hop * a:hop * b].contiguous()) for a, b in ((0, cuts[0]), (cuts[0], cuts[1]), (cuts[1], M))] + [s.flush()]
        put(f"dn/{cid}/strength{strength}/session", *[p for p in pieces if p.numel()])
    edge = -(-(n_fft // 2) // hop)                              # frames on either side whose window leaves the signal
    if M + 1 - edge > edge:                                     # an interior frame exists: anything estimate_bias raises fails the run
        put(f"dn/{cid}/estimate_bias", dn.estimate_bias(wav[:1]))
print(json.dumps(out))
'''
args = [dsp_code, str(REPO)] if mode == "dsp" else [code, json.dumps(shapes), mode]
res = {}
for name, lib in (("release", None), ("ref", os.path.abspath(sys.argv[1]))):
    env = dict(os.environ)
    if lib: env["IRIS_HIFIGAN_LIB"] = lib
    else: env.pop("IRIS_HIFIGAN_LIB", None)
    p = subprocess.run([sys.executable, "-c", *args], env=env, capture_output=True, text=True)
    if p.returncode: print(p.stderr[-2000:]); sys.exit(1)
    res[name] = json.loads(p.stdout.strip().splitlines()[-1])
bad = [k for k in res["release"] if res["release"][k] != res["ref"].get(k)] + [k for k in res["ref"] if k not in res["release"]]
print(f"{len(res['release'])} {'outputs' if mode == 'dsp' else 'shapes'} compared bitwise; differing: {bad}")
if mode == "dsp" and len(sys.argv) > 3:
    Path(sys.argv[3]).write_text(json.dumps({
        "tool": "tools/bitwise_sweep.py <the parent commit's library> dsp", "release": "this tree's library", "ref": "the library built from the parent commit",
        "compared": len(res["release"]), "differing": len(bad), "differing_keys": {k: [res["release"].get(k), res["ref"].get(k)] for k in bad},
        "sha256": res["release"]}, indent=1) + "\n")
sys.exit(1 if bad else 0)
