#!/usr/bin/env python3
"""The bits of the fp16 and bf16x3 vocoders on a fixed list of small cases: one sha256 per case over the raw bytes of what the
call wrote (audio, mel buffers, seed buffers), as JSON.  For comparing two trees -- a host-path change must leave every hash as it
was: run it on each (a process per tree, one after the other) and compare the files.  No assertion of its own.

  python tools/vocoder_bits.py [--tree PATH] [--out FILE]      PATH: the (built) tree whose package is imported; default: this one

Cases, on the 12-flow synthetic vocoder of facppg/synth.py at hop 256 and hop 160 (kc = 560 is no multiple of 64):
  infer         a ragged batch of 3, lengths (40, 33, 7): frames past T_valid, a part-filled last tile; injected z and noise drawn
                by the call (seed 1, device-side lengths); every forced tile width and the default; fp16: both K orders
  seeded path   T = 75 at hop 256, T = 40 at hop 160: mel_pad; cond_seed with block_tiles 1 and the maximum, layers_per_workgroup 1
                and 2, a bounded launch with a counter, flows (3, 4) on a sentinel-filled buffer; infer_seeded with 0, 32 and 64
                seeded frames, on a layout for 200 frames, and with events for two flows"""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (40, 33, 7)
SEEDED = ((256, 75), (160, 40))
SENT = -7.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, "fac-via-ppg_amd")]
    import torch
    from facppg import lib as flib
    from facppg import synth
    from waveglow.glow import WaveGlow
    assert os.path.abspath(flib.__file__).startswith(tree + os.sep), flib.__file__
    dev = torch.device("cuda", 0)
    out = {}

    def put(name, t):
        torch.cuda.synchronize()
        out[name] = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()

    def model(hop, half):
        cfg = dict(synth.WAVEGLOW_CONFIG, hop_length=hop, n_flows=12)
        m = WaveGlow.remove_weightnorm(WaveGlow(**cfg))
        m.load_state_dict(synth.waveglow_state_dict(cfg), strict=True)
        m = m.cuda().eval()
        if half:
            m.half()
            for k in m.convinv:
                k.float()
        return m, cfg

    def force_tile(var, tile):
        os.environ.pop(var, None)
        if tile:
            os.environ[var] = str(tile)

    def infer_cases(arith, hop):
        half = arith == "fp16"
        m, cfg = model(hop, half)
        B, T = len(LENGTHS), max(LENGTHS)
        mel = synth.synthetic_mel(B, T, seed=31).cuda()
        mel = mel.half() if half else mel
        zs = synth.synthetic_z(B, T * hop // 8, cfg, seed=32)
        lt = torch.tensor(LENGTHS, dtype=torch.int32, device=dev)
        var, tiles = ("FACPPG_WG16_TILE", (0, 32, 64, 128)) if half else ("FACPPG_WG_SPLIT_TILE", (0, 32, 64))
        for tile in tiles:
            force_tile(var, tile)
            for cf in ((False, True) if half else (False,)):
                kw = {"cond_first": cf} if half else {"arithmetic": arith}
                tag = "%s/hop%d/infer/tile=%s/cond_first=%d" % (arith, hop, tile or "unset", cf)
                put(tag + "/z", m.infer(mel, sigma=0.6, z=zs, lengths=list(LENGTHS), **kw))
                put(tag + "/drawn", m.infer(mel, sigma=0.6, seed=1, lengths=lt, **kw))
        force_tile(var, 0)

    def seeded_cases(arith, hop, T):
        half = arith == "fp16"
        m, cfg = model(hop, half)
        kw = {} if half else {"arithmetic": arith}
        tag = "%s/hop%d/T%d/" % (arith, hop, T)
        mel = synth.synthetic_mel(1, T, seed=91).cuda()
        zs = synth.synthetic_z(1, T * hop // 8, cfg, seed=92)
        nbytes = m.seed_layout(T, dev, **kw)[2]
        melp = m.mel_pad(mel, **kw)
        put(tag + "mel_pad", melp)
        used = -(-T // 32)

        def buf(n=nbytes):
            return torch.full((n // 4,), SENT, dtype=torch.float32, device=dev)
        bt_max = 0
        for bt in (4, 3, 2, 1):            # the widest block the entry point takes (a refusal launches nothing)
            try:
                m.cond_seed(melp, T, 0, 32 * used, buf(), block_tiles=bt, layers_per_workgroup=1, **kw)
            except flib.FacppgError:
                continue
            bt_max = bt
            break
        out[tag + "max_block_tiles"] = bt_max
        a = buf()
        m.cond_seed(melp, T, 0, 32 * used, a, block_tiles=1, layers_per_workgroup=1, **kw)
        put(tag + "cond_seed/bt=1/lpw=1", a)
        for bt, lpw in ((1, 2), (bt_max, 1), (bt_max, 2)):
            b = buf()
            m.cond_seed(melp, T, 0, 32 * used, b, block_tiles=bt, layers_per_workgroup=lpw, **kw)
            put(tag + "cond_seed/bt=max%+d/lpw=%d" % (bt - bt_max, lpw), b)
        b = buf()
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        m.cond_seed(melp, T, 0, 32 * used, b, block_tiles=bt_max, layers_per_workgroup=2, max_workgroups=64, counter=counter, **kw)
        put(tag + "cond_seed/bounded", b)
        b = buf()
        m.cond_seed(melp, T, 32, 32, b, block_tiles=1, flows=(3, 4), **kw)
        put(tag + "cond_seed/flows=3+4/frames=32+32", b)
        del b
        for s in (0, 32, 64):
            put(tag + "infer_seeded/seeded=%d/z" % s, m.infer_seeded(melp, T, a, s, sigma=0.6, z=zs, **kw))
        put(tag + "infer_seeded/seeded=32/drawn", m.infer_seeded(melp, T, a, 32, sigma=0.6, seed=1, **kw))
        evs = {}
        for k in (cfg["n_flows"] - 1, 5):
            evs[k] = torch.cuda.Event()
            evs[k].record()
        put(tag + "infer_seeded/seeded=64/flow_events", m.infer_seeded(melp, T, a, 64, sigma=0.6, z=zs, flow_events=evs, **kw))
        del a
        tqp2, _, nbytes2 = m.seed_layout(200, dev, **kw)[:3]
        melp2 = torch.zeros(tqp2, 80, dtype=melp.dtype, device=dev)
        m.mel_convert(mel[0].contiguous(), 200, 0, T, melp2, **kw)
        put(tag + "T_layout=200/mel_convert", melp2)
        a2 = buf(nbytes2)
        m.cond_seed(melp2, 200, 0, 32 * used, a2, block_tiles=bt_max, **kw)
        put(tag + "T_layout=200/cond_seed", a2)
        put(tag + "T_layout=200/infer_seeded/seeded=32", m.infer_seeded(melp2, T, a2, 32, sigma=0.6, z=zs, T_layout=200, **kw))

    with torch.no_grad():
        for arith in ("fp16", "bf16x3"):
            for hop in (256, 160):
                infer_cases(arith, hop)
            for hop, T in SEEDED:
                seeded_cases(arith, hop, T)
    text = json.dumps({"cases": out}, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
