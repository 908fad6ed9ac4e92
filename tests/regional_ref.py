"""The reference of the regional-conditioning tests: upstream ComfyUI's get_area_and_mult and the accumulate / divide loops of calc_cond_batch,
restated in plain torch, operation by operation, with Python slices and the `for t in range(8)` ramps — as upstream writes them, not as
lightdiffusion_amd.ops evaluates them.  An entry is lightdiffusion_amd.ops.RegionalEntry (list, group, slot, area (h, w, y0, x0), strength, mask
[Bm, H, W] or None, mask_strength); its model output is rows [slot * B, (slot + 1) * B) of outs[group].  Everything runs on the host in fp32:
IEEE products, sums and divisions, each rounded on its own."""
import torch


def get_area_and_mult(entry, x_in):
    """-> (area, mult): mult [B, C, h, w] as upstream builds it for one entry"""
    h, w, y0, x0 = entry.area
    area = (h, w, y0, x0)
    input_x = x_in[:, :, y0:y0 + h, x0:x0 + w]
    if entry.mask is not None:
        mask = entry.mask
        assert mask.shape[1:] == x_in.shape[2:]
        mask = mask[:, y0:y0 + h, x0:x0 + w] * entry.mask_strength
        mask = mask.unsqueeze(1).repeat(input_x.shape[0] // mask.shape[0], input_x.shape[1], 1, 1)
    else:
        mask = torch.ones_like(input_x)
    mult = mask * entry.strength
    if entry.mask is None:
        rr = 8
        if area[2] != 0:
            for t in range(rr):
                mult[:, :, t:1 + t, :] *= ((1.0 / rr) * (t + 1))
        if (area[0] + area[2]) < x_in.shape[2]:
            for t in range(rr):
                mult[:, :, area[0] - 1 - t:area[0] - t, :] *= ((1.0 / rr) * (t + 1))
        if area[3] != 0:
            for t in range(rr):
                mult[:, :, :, t:1 + t] *= ((1.0 / rr) * (t + 1))
        if (area[1] + area[3]) < x_in.shape[3]:
            for t in range(rr):
                mult[:, :, :, area[1] - 1 - t:area[1] - t] *= ((1.0 / rr) * (t + 1))
    return area, mult


def calc_cond_batch(outs, entries, shape):
    """-> [cond_pred, uncond_pred]: out_conds / out_counts of upstream, the entries accumulated in the order given"""
    b = shape[0]
    x_in = torch.zeros(shape)
    out_conds = [torch.zeros_like(x_in), torch.zeros_like(x_in)]
    out_counts = [torch.ones_like(x_in) * 1e-37, torch.ones_like(x_in) * 1e-37]
    for e in entries:
        a, mult = get_area_and_mult(e, x_in)
        output = outs[e.group][e.slot * b:(e.slot + 1) * b]
        out_conds[e.list][:, :, a[2]:a[0] + a[2], a[3]:a[1] + a[3]] += output * mult
        out_counts[e.list][:, :, a[2]:a[0] + a[2], a[3]:a[1] + a[3]] += mult
    for i in range(2):
        out_conds[i] /= out_counts[i]
    return out_conds


def combine(outs, entries, cond_scale, shape):
    """what ops.regional_combine computes: cfg_function on calc_cond_batch's two predictions"""
    cond_pred, uncond_pred = calc_cond_batch([o.cpu() for o in outs], [e._replace(mask=None if e.mask is None else e.mask.cpu()) for e in entries], shape)
    return uncond_pred + (cond_pred - uncond_pred) * cond_scale


def gather(x, windows):
    """what ops.regional_gather computes: the windows' slices of x, concatenated along the batch"""
    return torch.cat([x[:, :, y0:y0 + h, x0:x0 + w] for h, w, y0, x0 in windows])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
