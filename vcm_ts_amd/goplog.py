"""The per-GOP log of the file loops: small rows that are made on the device, on the stream that codes a picture, and that
the host looks at only when a GOP -- or the whole sequence -- is done.

    log.add(key, row=None)    one more row, keyed by its frame or step number; it is on the device already
    log.flush(*bufs)          the rows since the last flush go to pinned host memory: ONE pinned allocation and ONE asynchronous
                              copy per tensor, ONE event, all on the current stream; no kernel but the stack, nothing waited for
    log.poll(wait=False)      [(keys, host tensors)] of the flushes whose copies have run since the last call, oldest first
    log.collect()             poll(wait=True): waits for every flush

The rows either come with add() and are stacked by flush(), or live in buffers of the caller's, written in place, of which
flush(*bufs) is handed the filled part (a None among them stays None).  The device tensors are kept until their copy has
run, and a flush without rows does nothing at all: a log that is never added to makes no pinned memory and no event.
"""
from __future__ import annotations


class GopLog:
    def __init__(self):
        self.keys, self.rows, self.done = [], [], []

    def add(self, key, row=None):
        """Returns the number of rows waiting."""
        self.keys.append(key)
        if row is not None:
            self.rows.append(row)
        return len(self.keys)

    def flush(self, *bufs):
        import torch

        if not self.keys:
            return
        devs = bufs or (torch.stack(self.rows),)
        hosts = [None if dev is None else torch.empty(dev.shape, dtype=dev.dtype).pin_memory() for dev in devs]
        for host, dev in zip(hosts, devs):
            if dev is not None:
                host.copy_(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(devs[0].device))
        self.done.append((ev, hosts, devs, self.keys))
        self.keys, self.rows = [], []

    def poll(self, wait=False):
        out = []
        while self.done and (wait or self.done[0][0].query()):
            ev, hosts, _, keys = self.done.pop(0)
            ev.synchronize()
            out.append((keys, hosts))
        return out

    def collect(self):
        return self.poll(wait=True)
