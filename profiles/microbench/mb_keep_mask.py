"""What drawing the keep masks on the device is worth (voxvae.set_mask_source): steps/s of fit and of the
getEval(missing_prob=0.5) loop at 32^3, B = 256, bf16, the VAE class with dropout=True, batches from deviceDataLoader -- so the mask is
the only host-to-device copy of an iteration.  Legs:

    parent_host   the parent commit's tree (host draw), when --parent names a checkout of it with its library built
    host          this tree, mask source 'host' (the default): must sit on parent_host, within the run-to-run spread
    device        this tree, mask source 'device'

Every leg is a fresh child process (one model, WARM warm-up iterations, STEPS[...] timed ones between two synchronisations); the legs are
interleaved REPEATS times in one session on one device, and every repeat is kept, with the median and the min..max spread.

    python profiles/microbench/mb_keep_mask.py [--parent PATH] [out.json]        (default out: profiles/keep_mask_ab.json)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARM, REPEATS = 20, 3
STEPS = {'fit': 400, 'getEval': 1000}              # about a second of device work per timed window
D, LZ, B, SPLIT = 32, 64, 256, 1024


def child(tree, source):
    sys.path.insert(0, os.path.join(tree, 'anytime-3d-reconstruction_amd'))
    import numpy as np
    import torch
    import voxvae
    from voxvae import synthetic as syn
    voxvae.set_default_dtype('bf16')
    voxvae.set_default_device('cuda:0')
    if source != 'host':                                  # the parent's tree has no switch: 'host' is all it can do
        voxvae.set_mask_source(source)
        voxvae.manual_seed(1)
    np.random.seed(0)
    import src.module.nolbo as nolbo
    from src.dataset_loader.modelnet_dataset import deviceDataLoader
    cfg = syn.make_config(D, LZ, True)
    model = nolbo.nolboSingleObject_modelnet_category_VAE(nolbo_structure=cfg, dropout=True, learning_rate=1e-4)
    model._encoder.set_weights_dict(syn.make_encoder_params(cfg['encoder']))
    model._decoder.set_weights_dict(syn.make_decoder_params(cfg['decoder']))
    loader = deviceDataLoader('synthetic:%d:%d' % (SPLIT, D), 'train', voxel=D, seed=0)
    cats = torch.from_numpy(syn.make_category_vectors(40, LZ)).to('cuda:0')

    def fit():
        x = loader.getNextBatch(B)['input_images']
        model.fit((x, x))

    def evaluate():
        b = loader.getNextBatch(B)
        model.getEval((b['input_images'], b['input_images'], b['class_list']), category_vectors=cats, missing_prob=0.5)

    out = {}
    for name, step in (('fit', fit), ('getEval', evaluate)):
        for _ in range(WARM):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS[name]):
            step()
        torch.cuda.synchronize()
        out[name + '_steps_per_s'] = STEPS[name] / (time.perf_counter() - t0)
    print('RESULT ' + json.dumps(out), flush=True)


def run_leg(tree, source):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', tree, source], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError('leg %s of %s failed (%d): %s' % (source, tree, r.returncode, r.stderr[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])


def main(argv):
    parent = None
    if '--parent' in argv:
        i = argv.index('--parent')
        parent = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    dest = argv[0] if argv else os.path.join(ROOT, 'profiles', 'keep_mask_ab.json')
    legs = ([('parent_host', parent, 'host')] if parent else []) + [('host', ROOT, 'host'), ('device', ROOT, 'device')]
    runs = {name: [] for name, _, _ in legs}
    for _ in range(REPEATS):                              # interleaved: a drift of the box lands on every leg alike
        for name, tree, source in legs:
            runs[name].append(run_leg(tree, source))
    import torch
    out = {'workload': dict(voxel=D, latent=LZ, batch=B, dtype='bf16', model='nolboSingleObject_modelnet_category_VAE(dropout=True)',
                            loader='deviceDataLoader', warmup=WARM, steps=STEPS, repeats=REPEATS),
           'device': torch.cuda.get_device_name(0), 'legs': {}}
    if not parent:
        out['legs']['parent_host'] = 'not measured (no --parent checkout given)'
    for name, rs in runs.items():
        leg = {}
        for key in rs[0]:
            v = sorted(r[key] for r in rs)
            leg[key] = dict(median=v[len(v) // 2], min=v[0], max=v[-1], spread_percent=100.0 * (v[-1] - v[0]) / v[len(v) // 2], repeats=[r[key] for r in rs])
        out['legs'][name] = leg
    text = json.dumps(out, indent=1)
    print(text)
    with open(dest, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--child':
        child(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1:])
