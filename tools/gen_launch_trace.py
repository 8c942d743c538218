"""The ordered kernel launches of one tiny generation per mode, for comparing two builds of the library.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/gen_launch_trace.py
    python tools/gen_launch_trace.py list DIR OUT.txt      # tools/linear_launch_trace.py's listing: "name grid=(..) wg=(..)" per launch, in start order, repeated blocks folded

Without arguments, greedy, at Zonos-v0.1 dimensions (the persistent kernels serve the first two): a guided batch 1; cfg_scale = 1; generate_batch() of three guided
requests with budgets of their own (a row table) and audio prefixes of 0, 3 and 5 frames; a mixed generate_batch() of two unguided requests and one guided pair; a
serve() session of two slots over three requests - two admissions, a retirement and a re-admission.  ZONOS_HIP_LIB selects the library."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run():
    import torch
    from zonos_amd import synth
    from zonos_amd.model import GenRequest
    from zonos_amd.testing import build_model
    cfg, dev, greedy = synth.FULL_CFG, "cuda:0", {"temperature": 0.0}
    d = cfg["d_model"]
    model, _ = build_model(cfg, 1, dev)

    def utt(name, halves, L):
        return synth.conditioning(11, name, halves, L, d).to(dev)

    def prefix(name, P):
        return torch.from_numpy(synth.randint(11, name, (1, 9, P), 1024)) if P else None

    def done(mode, outs):
        torch.cuda.synchronize()
        print("mode", mode, "-> codes checksums", [int(o.sum()) for o in outs if o is not None], flush=True)

    done("guided batch 1", [model.generate(utt("g1", 2, 6), max_new_tokens=20, cfg_scale=2.0, sampling_params=greedy)])
    done("cfg_scale 1", [model.generate(utt("u1", 1, 6), max_new_tokens=20, cfg_scale=1.0, sampling_params=greedy)])
    reqs = [GenRequest(utt("r%d" % b, 2, 5 + b), dict(temperature=0.0, repetition_penalty=2.0 + b), seed=b, cfg_scale=2.0 + b, max_new_tokens=10 + b,
                       audio_prefix_codes=prefix("p%d" % b, (0, 3, 5)[b])) for b in range(3)]
    done("row table, unequal prefixes", model.generate_batch(reqs, ragged_prefix=True))
    mixed = [GenRequest(utt("m0", 1, 5), dict(greedy), seed=1, cfg_scale=1.0, max_new_tokens=9), GenRequest(utt("m1", 2, 6), dict(greedy), seed=2, cfg_scale=2.0, max_new_tokens=11),
             GenRequest(utt("m2", 1, 4), dict(greedy), seed=3, cfg_scale=1.0, max_new_tokens=10)]
    done("mixed, one pair", model.generate_batch(mixed, mixed_guidance=True))
    queue = [GenRequest(utt("s%d" % b, 2, 5 + b), dict(greedy), seed=b, cfg_scale=2.0, max_new_tokens=(6, 30, 8)[b]) for b in range(3)]
    got = sorted(model.serve(queue, slots=2, max_prompt=16, max_new_tokens=32, guided=True, sched_every=8), key=lambda r: r.index)
    assert all(r.error is None for r in got), [r.error for r in got]
    done("session: two admissions, a retire, a re-admission", [r.codes for r in got])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "list":
        from linear_launch_trace import listing
        listing(sys.argv[2], sys.argv[3])
    else:
        run()
