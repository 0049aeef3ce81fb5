"""Referee for cgck_steer / cgck_rss_steer_desc: the stable partition by queue id
of include/cgck.h, section 3, restated in numpy.  bucket_loop() is the same
contract as a naive Python loop, which test_steer_cpu.py holds expect() against.
Nothing here calls the library under test."""
import numpy as np


def bins(queue, queue_num):
    """bin(k): queue[k] below queue_num, else the unsteered bin queue_num."""
    queue = np.asarray(queue, np.uint8).astype(np.int64)
    return np.where(queue < queue_num, queue, queue_num)


def expect(queue, queue_num, desc=None):
    """(qoff u32[queue_num + 2], perm u32[n], slot u32[n], desc_out or None)."""
    b = bins(queue, queue_num)
    n = len(b)
    perm = np.argsort(b, kind="stable").astype(np.uint32)
    slot = np.empty(n, np.uint32)
    slot[perm] = np.arange(n, dtype=np.uint32)
    counts = np.bincount(b, minlength=queue_num + 1)
    qoff = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
    assert len(qoff) == queue_num + 2 and int(qoff[-1]) == n
    return qoff, perm, slot, None if desc is None else np.asarray(desc)[perm]


def bucket_loop(queue, queue_num):
    """(qoff, perm, slot) by appending each frame to its bin's list in arrival order."""
    buckets = [[] for _ in range(queue_num + 1)]
    for k, q in enumerate(queue):
        buckets[int(q) if int(q) < queue_num else queue_num].append(k)
    qoff, perm = [0], []
    for bucket in buckets:
        perm += bucket
        qoff.append(len(perm))
    slot = [0] * len(perm)
    for s, k in enumerate(perm):
        slot[k] = s
    return qoff, perm, slot
