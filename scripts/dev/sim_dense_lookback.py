#!/usr/bin/env python3
"""Model of encode_dense_kernel's ordered hand-off: why the tail of the tile
latency, not the ticket or the hop count, sets the rate.

S workgroup slots work through N tiles in ticket order. A tile takes a slot, needs `work` us to
load and size its units (median --work, a lognormal tail of --sigma), publishes its aggregate,
and may finish only when every earlier tile has published (+ --hop us per look-back hop of 64
tiles back to the newest inclusive prefix, + --store us to write its bytes). While it waits it
keeps its slot. Prints tiles/us and the mean wait for a few slot counts; --sigma 0 shows the
rate without a tail (slots / (work + hop + store)).
"""
import argparse
import heapq

import numpy as np


def run(n, slots, work, sigma, hop, store, ticket, seed=1):
    rng = np.random.default_rng(seed)
    w = work * np.exp(sigma * rng.standard_normal(n))
    free = [0.0] * slots          # when each slot is free again
    heapq.heapify(free)
    pub_max = 0.0                 # latest aggregate publication among tiles 0 .. t - 1
    incl = []                     # publication times of inclusive prefixes, in tile order
    t_ticket = 0.0
    waits = 0.0
    end = 0.0
    for t in range(n):
        start = max(heapq.heappop(free), t_ticket)
        t_ticket = start + ticket                  # one ticket word: tickets are serial
        agg = start + w[t]
        ready = max(agg, pub_max)                  # every earlier aggregate is out
        # hops back to the newest inclusive prefix published by then
        k = t
        while k > 0 and incl[k - 1] > ready:
            k -= 1
        hops = max(1, -(-(t - k + 1) // 64)) if t else 0
        done_lb = ready + hops * hop
        incl.append(done_lb)
        pub_max = max(pub_max, agg)
        waits += done_lb - agg
        fin = done_lb + store
        end = max(end, fin)
        heapq.heappush(free, fin)
    return n / end, waits / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=20000)
    ap.add_argument("--work", type=float, default=6.0, help="median us from ticket to aggregate")
    ap.add_argument("--sigma", type=float, default=0.6, help="lognormal sigma of that time")
    ap.add_argument("--hop", type=float, default=2.0, help="us per look-back hop")
    ap.add_argument("--store", type=float, default=3.0, help="us from offset to the end of the write-back")
    ap.add_argument("--ticket", type=float, default=0.0114, help="us per ticket (88 per us)")
    a = ap.parse_args()
    for slots in (256, 512, 768, 1536, 3072):
        for sigma in (0.0, a.sigma):
            rate, wait = run(a.tiles, slots, a.work, sigma, a.hop, a.store, a.ticket)
            print(f"slots {slots:5d}  sigma {sigma:.1f}: {rate:6.1f} tiles/us, mean wait {wait:6.1f} us")


if __name__ == "__main__":
    main()
