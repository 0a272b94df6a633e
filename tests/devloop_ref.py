"""numpy reference of the episode rule of trpo_ctx_record_episodes_dev (include/trpo_mi355x.h): flags
[num_env][slot_rows]; an episode ends at the first step with either flag set."""
import numpy as np


def episodes(terminated, truncated, num_env, slot_rows):
    """(ep_len [num_env] uintp, boot [num_env] uint8); truncated may be None"""
    term = np.asarray(terminated, np.uint8).reshape(num_env, slot_rows) != 0
    trun = np.zeros_like(term) if truncated is None else np.asarray(truncated, np.uint8).reshape(num_env, slot_rows) != 0
    hit = term | trun
    found = hit.any(axis=1)
    first = np.where(found, hit.argmax(axis=1), slot_rows - 1)
    ep_len = (first + 1).astype(np.uintp)
    boot = np.where(found, ~term[np.arange(num_env), first], True).astype(np.uint8)
    return ep_len, boot


def episodes_loop(terminated, truncated, num_env, slot_rows):
    """the same by the definition, one step at a time"""
    ep_len, boot = np.zeros(num_env, np.uintp), np.zeros(num_env, np.uint8)
    for e in range(num_env):
        ep_len[e], boot[e] = slot_rows, 1
        for t in range(slot_rows):
            a = terminated[e * slot_rows + t] != 0
            b = truncated is not None and truncated[e * slot_rows + t] != 0
            if a or b:
                ep_len[e], boot[e] = t + 1, 0 if a else 1
                break
    return ep_len, boot
