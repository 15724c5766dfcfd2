"""Per-iteration view of one LOAM scan2map (65 536 x 1 M, 10 iterations): cache hits / searches per linearisation (trace) and the
in-kernel timeline of every launch (pcr_params.record_timeline = 1)."""
import sys, numpy as np
sys.path.insert(0, '.')
import torch
from simpleslam_amd import LoamRegister, synth, pcr
S = 20261003 + 2
w, m = synth.make_map(1_000_000, seed=S)
scan, T = synth.make_scan(w, 0, seed=S)
T0 = synth.perturb(T, S)
dm, ds = torch.from_numpy(m).cuda(), torch.from_numpy(scan).cuda()
p = pcr.default_params(loam_iters=10, loam_early_exit=0, record_trace=1)
reg = LoamRegister(params=p)
pose = T0.copy(); reg.scan2Map(ds, dm, pose)
tr = reg.trace()
print('accepted rows  ', tr['n'])
print('cache hits     ', tr['cache_hits'])
print('searches       ', tr['searches'])
p = pcr.default_params(loam_iters=10, loam_early_exit=0)
p.record_timeline = 1
reg = LoamRegister(params=p)
for i in range(3):
    pose = T0.copy(); reg.scan2Map(ds, dm, pose)
tl = reg.timeline()
names = ['entry', 'prologue', 'posted', 'searched', 'plane', 'accum', 'stored']
for k in range(tl.shape[0]):
    t = tl[k]; ok = t[:, 6] > 0
    d = np.diff(t[ok][:, :7], axis=1).mean(axis=0)
    print(k, ' '.join(f'{names[i + 1]}:{d[i]:6.2f}' for i in range(6)), f'| mean stored {t[ok, 6].mean():6.2f} max stored {t[ok, 6].max():6.2f}')
# the head of a launch ('prologue' above: entry -> prologue stamp), split by the stamps inside it (launch 0 has no previous launch to fold)
print('head, mean block, us:  partial sums arrived | solved | pose ready | whole head')
for k in range(1, tl.shape[0]):
    t = tl[k]; ok = (t[:, 6] > 0) & (t[:, 7] > 0) & (t[:, 11] > 0)
    if ok.any():
        print(f'  launch {k}: ' + ' | '.join(f'{np.mean(t[ok, b] - t[ok, a]):5.2f}' for a, b in ((0, 7), (7, 11), (11, 1))) + f' | {np.mean(t[ok, 1] - t[ok, 0]):5.2f}')
t = tl[0]; ok = t[:, 10] > 0
if ok.any():
    for a, b, n in ((2, 8, 'ranges'), (8, 9, 'first group'), (9, 10, 'stream'), (10, 3, 'decode + exchange')):
        print(f'  launch 0 dense search: {n:18s} {np.mean(t[ok, b] - t[ok, a]):6.2f} us')
# the refine + plane stage ('plane' above: searched -> entry stamp), split by the stamps inside it
sub = (('gather', 3, 12), ('dist+sort+proof', 12, 13), ('plane fit', 13, 14), ('plane gate', 14, 15), ('entry', 15, 4))
print('refine + plane stage, mean block, us:  ' + ' | '.join(n for n, _, _ in sub) + ' | whole stage')
for k in range(min(4, tl.shape[0])):
    t = tl[k]; ok = (t[:, 6] > 0) & (t[:, 12] > 0)
    if ok.any():
        print(f'  launch {k}: ' + ' | '.join(f'{np.mean(t[ok, b] - t[ok, a]):5.2f}' for _, a, b in sub) + f' | {np.mean(t[ok, 4] - t[ok, 3]):5.2f}')
# the body around the search: 'posted' (prologue -> posted) and 'accum' + 'stored' (plane -> accum -> stored), split by the stamps inside them
sub = (('pose in registers', 1, 16), ('hit test', 16, 17), ('posting', 17, 2), ('rows to LDS', 4, 18), ('chunk sums', 18, 19), ('entry stores', 19, 5),
       ('block row', 5, 6))
print('post / accumulate / store stages, mean block, us:  ' + ' | '.join(n for n, _, _ in sub) + ' | mean block end')
for k in range(tl.shape[0]):
    t = tl[k]; ok = (t[:, 6] > 0) & (t[:, 18] > 0)
    if ok.any():
        print(f'  launch {k}: ' + ' | '.join(f'{np.mean(t[ok, b] - t[ok, a]):5.2f}' for _, a, b in sub) + f' | {t[ok, 6].mean():6.2f}')
# solved -> query transformed, split by the stamps inside it, in the order thread 0 passes them: 21 the wave's LDS-DMA has landed, 22 entry in
# registers, 23 the prologue's closing barrier (which also frees the staging area), 1 prologue left, 20 pose in registers, 16 query transformed
# (launch 0 fetches no entry: 21 and 22 are not taken there, and its stretch starts at the kernel's entry)
names = {1: 'prologue left', 20: 'pose in regs', 21: 'DMA landed', 22: 'entry read', 23: 'barrier', 16: 'transformed'}
print('solved -> query transformed, mean block, us (each stamp: time since the one before it)')
for k in range(tl.shape[0]):
    t = tl[k]; ok = (t[:, 6] > 0) & (t[:, 16] > 0)
    if not ok.any():
        continue
    start = 11 if k else 0
    at = sorted((np.mean(t[ok, s] - t[ok, start]), s) for s in names if (t[ok, s] > 0).all())
    prev, cells = 0.0, []
    for v, s in at:
        cells.append(f'{names[s]}:{v - prev:5.2f}'); prev = v
    print(f'  launch {k}: ' + ' | '.join(cells) + f' | whole stretch {prev:5.2f}')
import hashlib
print('pose sha1', hashlib.sha1(np.ascontiguousarray(pose).tobytes()).hexdigest())
reg.set_profile(2)
pose = T0.copy(); reg.scan2Map(ds, dm, pose)
print(reg.stats())
