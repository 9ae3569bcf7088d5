"""Helpers of the isoform-consensus tests: fixtures (reference GTFs), a random stage input, and plain numpy references of
the two device calls (consensus counts, boundary votes)."""
import gzip
import json
import os
import random

import numpy as np

import goldens

ISO_DIR = os.path.join(goldens.GOLDEN_DIR, "isoforms")


def names():
    return sorted(f[:-8] for f in os.listdir(ISO_DIR) if f.endswith(".json.gz"))


def load(name):
    return json.loads(gzip.open(os.path.join(ISO_DIR, name + ".json.gz")).read().decode())


def settings():
    return [tuple(s) for s in json.load(open(os.path.join(ISO_DIR, "INDEX.json")))["settings"]]


def write_case(name, tmp_path, split_dir_of):
    """cluster dir + split dir of a fixture case; returns (doc, cluster_tsv, split_tsv)."""
    doc = load(name)
    d, contig, tid = split_dir_of(name, tmp_path)
    cdir = os.path.join(str(tmp_path), "cluster_" + name, contig)
    os.makedirs(cdir, exist_ok=True)
    ctsv = os.path.join(cdir, "cluster_%s_%d.tsv" % (contig, tid))
    open(ctsv, "w").write(doc["cluster_tsv"])
    return doc, ctsv, os.path.join(d, contig, "split_%s_%d.tsv" % (contig, tid)), os.path.dirname(cdir), d


def random_job(seed, n_iso, reads_per_iso, n_segs, tail_p=0.3):
    """(isoforms, segments, reads) as read_cluster() + read_split() leave them, without files."""
    rng = random.Random(seed)
    pos = [1000 + 37 * j + rng.randrange(5) for j in range(n_segs + 1)]
    pos = sorted(set(pos))
    while len(pos) < n_segs + 1:
        pos.append(pos[-1] + 30)
    segs = list(zip(pos[:-1], pos[1:]))
    segments = {("c", seed): segs}
    reads, isoforms = {}, {}
    rid = 0
    for iid in range(n_iso):
        pat = [1 if rng.random() < 0.5 else 0 for _ in range(n_segs)]
        key = ("c", seed, 0, iid)
        isoforms[key] = dict(rids=set())
        for _ in range(reads_per_iso if iid else 2):               # the first isoform is too small for any exon (x >= 3)
            a = rng.randrange(n_segs); b = rng.randrange(a, n_segs)
            data = "".join(str((pat[j] if rng.random() > 0.05 else 1 - pat[j]) if a <= j <= b else (2 if rng.random() < 0.02 else 0))
                           for j in range(n_segs))
            r = rng.random()
            tail = "S" if r < tail_p / 2 else ("E" if r < tail_p else "N")
            starts, ends = [], []
            for j in range(n_segs):
                if data[j] == "1" and (j == 0 or data[j - 1] != "1"):
                    starts.append(segs[j][0] + rng.randrange(-12, 13))
                if data[j] == "1" and (j == n_segs - 1 or data[j + 1] != "1"):
                    ends.append(segs[j][1] + rng.randrange(-12, 13))
            if not starts:
                starts, ends = [pos[0]], [pos[0] + 1]
            reads[rid] = dict(rid=rid, rname="r%d" % rid, chrom="c", strand="+", tint=seed, pid=0, tail=tail, iid=iid, data=data,
                              starts=tuple(starts), ends=tuple(ends))
            isoforms[key]["rids"].add(rid)
            rid += 1
    return isoforms, segments, reads


def plain_counts(iro, n_seg, off, lab, tail):
    """cons / cov / tails of isoforms_cons (:203-232) with numpy, an isoform at a time; a read's row is lab[off[r]:off[r] + M],
    wherever that lies."""
    cons, cov, tails = [], [], []
    for i in range(len(n_seg)):
        M, r0, r1 = int(n_seg[i]), int(iro[i]), int(iro[i + 1])
        rows = np.stack([lab[int(off[r]):int(off[r]) + M] for r in range(r0, r1)]) if r1 > r0 and M else np.zeros((r1 - r0, M), np.uint8)
        one = rows == ord("1")
        has = one.any(1) if M else np.zeros(r1 - r0, bool)
        first = np.where(has, one.argmax(1), M) if M else np.zeros(r1 - r0, int)
        last = np.where(has, M - 1 - one[:, ::-1].argmax(1), -1) if M else np.zeros(r1 - r0, int) - 1
        tl = tail[r0:r1]
        first = np.where(has & (tl == 1), 0, first); last = np.where(has & (tl == 1), M - 1, last)
        j = np.arange(M)[None, :]
        inside = (j >= first[:, None]) & (j <= last[:, None])
        cons.append((inside & one).sum(0)); cov.append(inside.sum(0))
        tails.append([int((has & (tl == k)).sum()) for k in range(3)])
    return np.concatenate(cons).astype(np.int32), np.concatenate(cov).astype(np.int32), np.asarray(tails, np.int32)


def plain_votes(iso_read_off, iso_b_off, iso_bound, read_b_off, read_bound, w):
    """votes of correct_boundaries (:129-137) as a (B, 2w + 1) int32 array: row = isoform boundary, column x + w = the
    member reads' boundaries at distance x from it.  Differences in int64, every x of the window counted: no search, no sort."""
    iso_bound = np.asarray(iso_bound, np.int64); read_bound = np.asarray(read_bound, np.int64)
    xs = np.arange(-w, w + 1, dtype=np.int64)
    out = np.zeros((int(iso_b_off[-1]), 2 * w + 1), np.int32)
    for i in range(len(iso_b_off) - 1):
        b0, b1 = int(iso_b_off[i]), int(iso_b_off[i + 1])
        q0, q1 = int(read_b_off[int(iso_read_off[i])]), int(read_b_off[int(iso_read_off[i + 1])])
        if b0 == b1 or q0 == q1:
            continue
        d = read_bound[None, q0:q1] - iso_bound[b0:b1, None]
        out[b0:b1] = (d[:, :, None] == xs[None, None, :]).sum(1)
    return out
