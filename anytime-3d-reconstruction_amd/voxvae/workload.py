"""Algorithmic work of the hot path per reconstruction: "valid" MACs count
only the filter taps that touch real data (TF 'SAME' zero padding skipped).  Used by bench.py's roofline leg."""


def _axis_pairs_s2(n_in):
    """(output, tap) pairs per axis of a k4 s2 SAME conv on n_in cells (= pairs of its transposed conv)."""
    return sum(1 for o in range(n_in // 2) for t in range(4) if 0 <= 2 * o - 1 + t < n_in)


def _axis_pairs_s1(n):
    """k4 s1 SAME (pad 1 before, 2 after)."""
    return sum(1 for o in range(n) for t in range(4) if 0 <= o - 1 + t < n)


def layer_macs(config):
    """-> list of (layer name, valid MACs per sample, dense-im2col MACs per sample)."""
    enc, dec = config['encoder'], config['decoder']
    out = []
    side, cin = enc['input_shape'][0], 1
    f = enc['filter_num_list']
    for i, c in enumerate(f[:-1]):
        out.append(('E%d' % (i + 1), _axis_pairs_s2(side) ** 3 * cin * c, (side // 2) ** 3 * 64 * cin * c))
        side, cin = side // 2, c
    out.append(('E%d' % len(f), _axis_pairs_s1(side) ** 3 * cin * f[-1], side ** 3 * 64 * cin * f[-1]))
    f = dec['filter_num_list']
    n = len(f)
    side = dec['output_shape'][0] >> (n - 1)
    ch = max(f[0] // 64, 8)
    out.append(('D0', dec['input_dim'] * side ** 3 * ch, dec['input_dim'] * side ** 3 * ch))
    out.append(('D1', _axis_pairs_s1(side) ** 3 * ch * f[0], side ** 3 * 64 * ch * f[0]))
    cin = f[0]
    for i in range(1, n):
        out.append(('D%d' % (i + 1), _axis_pairs_s2(2 * side) ** 3 * cin * f[i], side ** 3 * 64 * cin * f[i]))
        side, cin = 2 * side, f[i]
    return out


def flops_per_reconstruction(config):
    lm = layer_macs(config)
    return 2 * sum(v for _, v, _ in lm), 2 * sum(d for _, _, d in lm)


# ---- the image encoder (src/net_core/darknet.py): Conv2D k in {1, 3}, stride 1, SAME; MaxPool2D(2, 2, 'same') halves with ceil
DARKNET19_PLAN = [(32, 3), 'M', (64, 3), 'M', (128, 3), (64, 1), (128, 3), 'M', (256, 3), (128, 1), (256, 3), 'M',
                  (512, 3), (256, 1), (512, 3), (256, 1), (512, 3), 'M', (1024, 3), (512, 1), (1024, 3), (512, 1), (1024, 3)]
NOLBO_HEAD = ([1024, 1024, 1024], [3, 3, 3], 245)      # nolbo_test's head: filter_num_list, filter_size_list, output_dim


def _axis_pairs_2d(n, k):
    """(output, tap) pairs per axis of a k s1 SAME conv on n cells."""
    return sum(1 for o in range(n) for t in range(k) if 0 <= o - k // 2 + t < n)


def image_encoder_macs(rows, cols, head=NOLBO_HEAD, plan=None):
    """-> list of (layer name, valid MACs per image, dense MACs per image) for Darknet19 on a rows x cols image followed by a head
    (filter_num_list, filter_size_list, output_dim), or by none (head=None).  Names: B1.. backbone convolutions, H1.. head, HL its last 1x1."""
    out, cin, n = [], 3, 0
    for item in (DARKNET19_PLAN if plan is None else plan):
        if item == 'M':
            rows, cols = (rows + 1) // 2, (cols + 1) // 2
            continue
        c, k = item
        n += 1
        out.append(('B%d' % n, _axis_pairs_2d(rows, k) * _axis_pairs_2d(cols, k) * cin * c, rows * cols * k * k * cin * c))
        cin = c
    if head is not None:
        for i, (c, k) in enumerate(zip(head[0], head[1])):
            out.append(('H%d' % (i + 1), _axis_pairs_2d(rows, k) * _axis_pairs_2d(cols, k) * cin * c, rows * cols * k * k * cin * c))
            cin = c
        out.append(('HL', rows * cols * cin * head[2], rows * cols * cin * head[2]))
    return out
