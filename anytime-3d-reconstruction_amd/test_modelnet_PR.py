"""The precision / recall curve of the reconstructions over the test split: the loop of the reference's test_modelnet_VAE.py (:104-156)
with the threshold sweep of its notebooks (modelnetAE3.ipynb cell 2, saved by cell 3) accumulated on the device while the loop runs --
the probabilities never cross PCIe and no `_pred.npy` has to be written and re-read.
`python test_modelnet_PR.py --voxel 32 --batch 256 --dtype bf16 --missing-pr 0.3 --out-dir DIR [--pr-div 20] [--pr-full] [--per-category]
[--sampling K] [--device-data | --packed-data] [--dump-dir DIR2]` writes

    DIR/<missing_pr>_pr_preds.npy, .txt               the [len(thresholds) + div, 2] (precision, recall) table of cell 3
    DIR/<missing_pr>_pr_preds_corrected.npy, .txt     the same for the corrected prediction (missing_pr > 0)
    DIR/<missing_pr>_pr_preds_sampled.npy, .txt       --sampling K: for the sampled-mean reconstruction over K latents per object
    DIR/<missing_pr>_pr_preds_per_category.npy        --per-category: [40, rows, 2], one table per class

--pr-full sweeps the notebook's commented r1 + r2 + r3 list instead of the active r2 list.  The `div` thinning rows are the expectation
of the notebook's random mask (voxvae.prcurve.notebook_table).  --dump-dir also writes the arrays test_modelnet_VAE.py --dump-dir writes
(plus `<missing_pr>_pred_corrected.npy`), so a run can be cross-checked against the numpy route."""
import os
import sys

import numpy as np

import _entry_common as C
import voxvae
from src.dataset_loader.modelnet_dataset import dataLoader, deviceDataLoader
from voxvae.prcurve import notebook_curve, notebook_table

FIELDS = ('loss', 'pr', 'rc', 'c'), ('closs', 'cpr', 'crc', 'cc')
CLASSES = 40


def _options(ap):
    ap.add_argument('--pr-div', type=int, default=20, help='the notebook\'s `div` (cell 3 calls test(..., div=20))')
    ap.add_argument('--pr-full', action='store_true', help='the commented r1 + r2 + r3 threshold list instead of the active r2')
    ap.add_argument('--per-category', action='store_true', help='also keep one curve per class')
    ap.add_argument('--out-dir', default='.', help='where the tables are written')


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.array(a)


def save_table(out_dir, name, table):
    np.save(os.path.join(out_dir, name + '.npy'), table)
    np.savetxt(os.path.join(out_dir, name + '.txt'), table)


def evaluate(model, loader, missing_pr, batch_size, max_iter, category_vectors, div=20, full=False, per_category=False, sampling=0,
             out_dir='.', dump_dir=None, class_key='class_list'):
    """getPRCurve over one epoch; returns {'eval': the 8 running means of test_modelnet_VAE.py, 'tables': {file stem: table}}."""
    groups = CLASSES if per_category else 1
    curves = {'': notebook_curve(div, full, groups)}
    if missing_pr > 0:
        curves['_corrected'] = notebook_curve(div, full, groups)
    if sampling > 0:
        curves['_sampled'] = notebook_curve(div, full, groups)
    means = C.RunningMeans(eval=8)
    bar = C.Progress(width=5)
    dumps = {'_cl_label': [], '_gt': [], '_pred': [], '_pred_corrected': []}
    print('start training...')
    for epoch, position, total in C.epochs_of(loader, 1, 'batchStart'):
        bar.tic()
        batch = loader.getNextBatch(batchSize=batch_size)
        x, cl = batch['input_images'], batch[class_key]
        group = cl if per_category else None
        out = model.getPRCurve((x, x, cl), curves[''], category_vectors=category_vectors, missing_prob=missing_pr,
                               corrected=curves.get('_corrected'), group=group)
        if sampling > 0:
            model.getPRCurve((x, x), curves['_sampled'], sampling_num=sampling, group=group)
        means.add(eval=out[1:5] + out[6:10])
        if dump_dir is not None:
            dumps['_cl_label'].append(_host(cl))
            dumps['_gt'].append(_host(x))
            dumps['_pred'].append(_host(out[0]))
            if missing_pr > 0:
                dumps['_pred_corrected'].append(_host(out[5]))
        bar.toc()
        m = means['eval']
        bar.show(epoch, position, total, bar.group(zip(FIELDS[0], m[:4])) + ",", bar.group(zip(FIELDS[1], m[4:])))
        if C.stop_on_nan(means):
            return None
        if max_iter is not None and means.n >= max_iter:
            break
    print('')
    os.makedirs(out_dir, exist_ok=True)
    tables = {}
    for suffix, curve in curves.items():
        stem = str(missing_pr) + '_pr_preds' + suffix
        tables[stem] = notebook_table(curve, div)
        save_table(out_dir, stem, tables[stem])
        if per_category:
            tables[stem + '_per_category'] = np.stack([notebook_table(curve, div, group=g) for g in range(groups)])
            np.save(os.path.join(out_dir, stem + '_per_category.npy'), tables[stem + '_per_category'])
    if dump_dir is not None:
        os.makedirs(dump_dir, exist_ok=True)
        for suffix, parts in dumps.items():
            if parts:
                np.save(os.path.join(dump_dir, str(missing_pr) + suffix + '.npy'), np.concatenate(parts, axis=0))
    return {'eval': means['eval'], 'tables': tables}


def run(a):
    import src.module.nolbo as nolbo
    config = C.make_config(a.latent, a.voxel, True)
    model = nolbo.nolboSingleObject_modelnet_category_VAE(nolbo_structure=config, learning_rate=a.lr)
    if a.packed_data and not a.device_data:
        loader = dataLoader(data_path=a.dataset_path, trainortest='test', voxel=a.voxel, packed=True)
    else:
        loader = (deviceDataLoader if a.device_data else dataLoader)(data_path=a.dataset_path, trainortest='test', voxel=a.voxel)
    category_vectors = None
    if a.load_path is not None:
        print('load weights...')
        model.loadModel(load_path=a.load_path)
        print('done!')
        cv = os.path.join(a.load_path, 'category_vectors.npy')
        if os.path.exists(cv):
            category_vectors = np.load(cv).astype('float32')
    if category_vectors is None:                                  # no prototypes on disk: seeded stand-ins
        from voxvae import synthetic as syn
        category_vectors = syn.make_category_vectors(CLASSES, config['z_category_dim'])
    return evaluate(model, loader, a.missing_pr, a.batch, a.max_iter, category_vectors, div=a.pr_div, full=a.pr_full,
                    per_category=a.per_category, sampling=a.sampling, out_dir=a.out_dir, dump_dir=a.dump_dir)


if __name__ == '__main__':
    a = C.parse(__doc__, extra=_options)
    if a.pipeline > 1:
        sys.exit('test_modelnet_PR.py runs the synchronous loop: use --pipeline 1')
    voxvae.set_default_dtype(a.dtype)
    sys.exit(0 if run(a) is not None else 1)
