"""`yttm` command line on top of the MI355X core: same commands and flags as the reference CLI
(youtokentome/yttm_cli.py:10-169: bpe | encode | decode | vocab), same stdout formats as the reference's native CLI
loops (bpe.cpp:1942-2028, utils.h:92-103).  Run as `python -m youtokentome_amd.yttm_cli ...`.

Two more commands work file to file through the device, with the same bytes as the streaming ones: `encode_file` (--output_type id: binary
PREFIX.ids / PREFIX.off; subword and id_text: the text `encode --output_type subword` / `id` prints) and `decode_file` (a file of decimal ids
-> the text `decode` prints).  `count_file` prints how often a text file uses every token, counted on the device: the lines of `vocab` with a
third column.  `encode`, `encode_file` and `count_file` take `--vocabulary FILE --vocabulary_threshold N`: FILE is what `count_file` wrote, and tokens
it counts fewer than N times are split back into smaller pieces (subword-nmt's --vocabulary / --vocabulary-threshold).  `encode`, `encode_file`,
`count_file`, `blocks_file`, `decode` and `decode_file` take `--byte_fallback`: characters outside the model's alphabet are the ids of their UTF-8
bytes, vocab_size + b, printed as <0xNN>, instead of one <UNK> per run (SentencePiece's byte_fallback).  The same six take `--added_tokens FILE`:
one token per line, literal strings that are matched in the text, never split, and are the ids vocab_size + 256 + line number (SentencePiece's
user_defined_symbols).

The loops themselves are C++ (youtokentome_amd/csrc/host_cli.cpp, behind yttm_encode_cli / yttm_decode_cli / yttm_vocab_cli):
stdin and stdout stay bytes end to end, invalid UTF-8 included."""

import click

from .bpe import _Core


@click.group()
def main():
    pass


def _vocabulary_options(f):
    f = click.option("--vocabulary_threshold", type=click.INT, default=1, show_default=True,
                     help="With --vocabulary: tokens the file counts fewer times than this are split into smaller pieces.")(f)
    return click.option("--vocabulary", type=click.Path(exists=True, dir_okay=False), required=False,
                        help="A file `count_file` wrote (id<TAB>subword<TAB>count): encode with the tokens it counts often enough only.")(f)


def _byte_fallback_option(f):
    return click.option("--byte_fallback", is_flag=True,
                        help="Characters outside the model's alphabet as the ids of their UTF-8 bytes (vocab_size + byte, <0xNN>) instead of <UNK>.")(f)


def _added_tokens_option(f):
    return click.option("--added_tokens", type=click.Path(exists=True, dir_okay=False), required=False,
                        help="A file of literal tokens, one per line: each is one id (vocab_size + 256 + its line number from 0) and never split.")(f)


def _set_added_tokens(core, path):
    """the tokens file -> the added tokens of the encoder: one per line, an empty line is an error"""
    if path is None:
        return
    with open(path, "rb") as f:
        data = f.read()
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # (the newline that ends the last line)
    for no, line in enumerate(lines, 1):
        if not line:
            raise click.ClickException("%s:%d: an empty line is no token" % (path, no))
    try:
        core.set_added_tokens(lines)
    except ValueError as e:
        raise click.ClickException("%s: %s" % (path, e))


def _set_vocabulary(core, path, threshold):
    """the vocabulary file -> the allowed set of the encoder; ids missing from the file count 0"""
    if path is None:
        return
    vocab = core.vocab()
    added = core.added_tokens_raw()
    counts = [0] * len(vocab)
    with open(path, "rb") as f:
        for no, line in enumerate(f.read().split(b"\n"), 1):
            if not line:
                continue
            cols = line.split(b"\t")
            try:
                if len(cols) != 3:
                    raise ValueError
                i, n = int(cols[0]), int(cols[2])
            except ValueError:
                raise click.ClickException("%s:%d: expected id<TAB>subword<TAB>count" % (path, no))
            if len(vocab) <= i < len(vocab) + 256 and cols[1] == b"<0x%02X>" % (i - len(vocab)):
                continue  # (a file `count_file --byte_fallback` wrote: a byte id is no token of the vocabulary, it is neither allowed nor split)
            if len(vocab) + 256 <= i < len(vocab) + 256 + len(added):
                if added[i - len(vocab) - 256] != cols[1]:
                    raise click.ClickException("%s:%d: id %d is not the added token %r: the vocabulary was counted with other added tokens" % (
                        path, no, i, cols[1].decode(errors="replace")))
                continue  # (a file `count_file --added_tokens` wrote: an added id is neither allowed nor split)
            if not 0 <= i < len(vocab) or vocab[i].encode() != cols[1]:
                raise click.ClickException("%s:%d: id %d is not this model's %r: the vocabulary belongs to another model" % (
                    path, no, i, cols[1].decode(errors="replace")))
            counts[i] = n
    core.set_vocabulary([n >= threshold for n in counts])


@main.command()
@click.option("--data", type=click.Path(exists=True), required=True, help="Training data file path.")
@click.option("--model", type=click.Path(), required=True, help="Output model file path.")
@click.option("--vocab_size", type=click.INT, required=True, help="Number of tokens in the final vocabulary.")
@click.option("--coverage", type=click.FLOAT, default=1.0, show_default=True, help="Percentage of characters covered by the model.")
@click.option("--n_threads", type=click.INT, default=-1, show_default=True, help="Number of threads (accepted, unused: the GPU trains).")
@click.option("--pad_id", type=click.INT, default=0, show_default=True, help="Padding token id.")
@click.option("--unk_id", type=click.INT, default=1, show_default=True, help="Unknown token id.")
@click.option("--bos_id", type=click.INT, default=2, show_default=True, help="Begin of sentence token id.")
@click.option("--eos_id", type=click.INT, default=3, show_default=True, help="End of sentence token id.")
def bpe(data, model, vocab_size, coverage, n_threads, pad_id, unk_id, bos_id, eos_id):
    """Train BPE model."""
    _Core.train(data=data, model=model, vocab_size=vocab_size, coverage=coverage, n_threads=n_threads, pad_id=pad_id,
                unk_id=unk_id, bos_id=bos_id, eos_id=eos_id)


@main.command()
@click.option("--model", type=click.Path(exists=True), required=True, help="Path to file with learned model.")
@click.option("--output_type", type=click.Choice(["id", "subword"]), required=True, help="'id' or 'subword'.")
@click.option("--n_threads", type=click.INT, default=-1, show_default=True, help="Number of threads.")
@click.option("--bos", is_flag=True, help="Add tab begin of sentence.")
@click.option("--eos", is_flag=True, help="Add tab end of sentence.")
@click.option("--reverse", is_flag=True, help="Reverse output sequence of tokens.")
@click.option("--stream", is_flag=True, help="Process each line before reading the next one.")
@click.option("--dropout_prob", type=click.FLOAT, default=0, show_default=True,
              help="BPE-dropout probability (the probability of a merge being dropped)")
@_vocabulary_options
@_byte_fallback_option
@_added_tokens_option
def encode(model, output_type, n_threads, bos, eos, reverse, stream, dropout_prob, vocabulary, vocabulary_threshold, byte_fallback, added_tokens):
    """Encode text to ids or subwords."""
    if n_threads < -1 or n_threads == 0:  # yttm_cli.py:110-114
        raise ValueError('Invalid value for "--n_threads": must be -1 or positive integer, not "%d"' % n_threads)
    core = _Core(model, n_threads)
    core.set_byte_fallback(byte_fallback)
    _set_added_tokens(core, added_tokens)
    _set_vocabulary(core, vocabulary, vocabulary_threshold)
    core.encode_cli(output_type, stream, bos, eos, reverse, dropout_prob)  # the C++ loop: yttm_encode_cli (host_cli.cpp)


@main.command(name="encode_file")
@click.option("--model", type=click.Path(exists=True), required=True, help="Path to file with learned model.")
@click.option("--input", "input_path", type=click.Path(exists=True, dir_okay=False), required=True, help="Text file, one sentence per line.")
@click.option("--output", type=click.Path(), required=True,
              help="Prefix of the output: PREFIX.ids (int32) and PREFIX.off (uint64), little-endian; with --output_type subword or id_text the text file to write.")
@click.option("--output_type", type=click.Choice(["id", "subword", "id_text"]), default="id", show_default=True,
              help="'id': binary ids and offsets; 'subword': the text `encode --output_type subword` prints; 'id_text': the text `encode --output_type id` prints.")
@click.option("--bos", is_flag=True, help="Add tab begin of sentence.")
@click.option("--eos", is_flag=True, help="Add tab end of sentence.")
@click.option("--reverse", is_flag=True, help="Reverse output sequence of tokens.")
@click.option("--dropout_prob", type=click.FLOAT, default=0, show_default=True,
              help="BPE-dropout probability (the probability of a merge being dropped)")
@_vocabulary_options
@_byte_fallback_option
@_added_tokens_option
def encode_file(model, input_path, output, output_type, bos, eos, reverse, dropout_prob, vocabulary, vocabulary_threshold, byte_fallback, added_tokens):
    """Encode a text file to binary ids and line offsets, or to a text file of subwords."""
    core = _Core(model)
    core.set_byte_fallback(byte_fallback)
    _set_added_tokens(core, added_tokens)
    _set_vocabulary(core, vocabulary, vocabulary_threshold)
    if output_type == "subword":  # the same pipeline with the formatter behind the encode: yttm_encode_file_subword (host_lines.cpp)
        core.encode_file_subword(input_path, output, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob)
        return
    if output_type == "id_text":  # ... with the id printer behind the encode: yttm_encode_file_idtext (host_lines.cpp)
        core.encode_file_idtext(input_path, output, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob)
        return
    core.encode_file(input_path, out=output, bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob)  # the C++ pipeline: yttm_encode_file (host_lines.cpp)


def _parse_ignore_ids(ctx, param, value):
    if value is None:
        return None
    try:
        return [int(v) for v in value.split(",")]
    except ValueError:
        raise click.BadParameter("Bad format: expected list of comma-separated integers, but got {}".format(value))


@main.command()
@click.option("--model", type=click.Path(exists=True), required=True, help="Path to file with learned model.")
@click.option("--ignore_ids", type=click.STRING, callback=_parse_ignore_ids, required=False,
              help="List of indices to ignore for decoding. Example: --ignore_ids=1,2,3")
@_byte_fallback_option
@_added_tokens_option
def decode(model, ignore_ids, byte_fallback, added_tokens):
    """Decode ids to text."""
    core = _Core(model)
    core.set_byte_fallback(byte_fallback)
    _set_added_tokens(core, added_tokens)
    core.decode_cli(ignore_ids)


@main.command(name="decode_file")
@click.option("--model", type=click.Path(exists=True), required=True, help="Path to file with learned model.")
@click.option("--input", "input_path", type=click.Path(exists=True, dir_okay=False), required=True, help="Text file of decimal ids, one sentence per line.")
@click.option("--output", type=click.Path(), required=True, help="The text file to write: what `decode` prints for the input.")
@click.option("--ignore_ids", type=click.STRING, callback=_parse_ignore_ids, required=False,
              help="List of indices to ignore for decoding. Example: --ignore_ids=1,2,3")
@_byte_fallback_option
@_added_tokens_option
def decode_file(model, input_path, output, ignore_ids, byte_fallback, added_tokens):
    """Decode a text file of ids to a text file."""
    core = _Core(model)
    core.set_byte_fallback(byte_fallback)
    _set_added_tokens(core, added_tokens)
    core.decode_file(input_path, output, ignore_ids=ignore_ids)  # the C++ pipeline: yttm_decode_file (host_lines.cpp)


@main.command(name="count_file")
@click.option("--model", type=click.Path(exists=True), required=True, help="Path to file with learned model.")
@click.option("--input", "input_path", type=click.Path(exists=True, dir_okay=False), required=True, help="Text file, one sentence per line.")
@click.option("--output", type=click.Path(), required=False, help="The file to write (default: stdout).")
@click.option("--bos", is_flag=True, help="Add tab begin of sentence.")
@click.option("--eos", is_flag=True, help="Add tab end of sentence.")
@click.option("--dropout_prob", type=click.FLOAT, default=0, show_default=True,
              help="BPE-dropout probability (the probability of a merge being dropped)")
@_vocabulary_options
@_byte_fallback_option
@_added_tokens_option
def count_file(model, input_path, output, bos, eos, dropout_prob, vocabulary, vocabulary_threshold, byte_fallback, added_tokens):
    """Print how often the file uses every token: id<TAB>subword<TAB>count, in id order."""
    import sys
    core = _Core(model)
    core.set_byte_fallback(byte_fallback)
    _set_added_tokens(core, added_tokens)
    _set_vocabulary(core, vocabulary, vocabulary_threshold)
    counts = core.encode_file_counts(input_path, bos=bos, eos=eos, dropout_prob=dropout_prob)  # the C++ pipeline: yttm_encode_file_counts (host_lines.cpp)
    # (the first two columns are those of `vocab`: the id and id_to_subword(id) as it stands)
    # (with --byte_fallback: 256 rows <0xNN> more; with --added_tokens those 256 rows whether the byte ids are in use or not, and a row per token)
    V, bound = core.vocab_size(), core.id_bound()
    pieces = core.vocab() + ["<0x%02X>" % (i - V) for i in range(V, min(bound, V + 256))] + [core.id_to_subword(i) for i in range(V + 256, bound)]
    text = b"".join(b"%d\t%s\t%d\n" % (i, piece.encode(), int(counts[i])) for i, piece in enumerate(pieces))
    if output is None:
        sys.stdout.flush()
        sys.stdout.buffer.write(text)
        sys.stdout.buffer.flush()
    else:
        with open(output, "wb") as f:
            f.write(text)


@main.command(name="blocks_file")
@click.option("--model", type=click.Path(exists=True), required=True, help="Path to file with learned model.")
@click.option("--input", "input_path", type=click.Path(exists=True, dir_okay=False), required=True, help="Text file, one sentence per line.")
@click.option("--output", type=click.Path(), required=True, help="Prefix of the files to write: PREFIX.rows (int32 [rows, seq_len]) and PREFIX.frags (uint64 [frags, 2]).")
@click.option("--seq_len", type=click.INT, required=True, help="Ids per row.")
@click.option("--mode", type=click.Choice(["stream", "whole"]), default="stream", show_default=True,
              help="stream: concatenate the sentences and cut every seq_len ids; whole: place sentences whole, several to a row.")
@click.option("--bos", is_flag=True, help="Add tab begin of sentence.")
@click.option("--eos", is_flag=True, help="Add tab end of sentence.")
@click.option("--reverse", is_flag=True, help="Reverse output sequence of tokens.")
@click.option("--dropout_prob", type=click.FLOAT, default=0, show_default=True,
              help="BPE-dropout probability (the probability of a merge being dropped)")
@click.option("--drop_last", is_flag=True, help="Discard the incomplete last row instead of padding it with <PAD>.")
@_vocabulary_options
@_byte_fallback_option
@_added_tokens_option
def blocks_file(model, input_path, output, seq_len, mode, bos, eos, reverse, dropout_prob, drop_last, vocabulary, vocabulary_threshold, byte_fallback, added_tokens):
    """Encode a text file and pack it into fixed-length training rows."""
    core = _Core(model)
    core.set_byte_fallback(byte_fallback)
    _set_added_tokens(core, added_tokens)
    _set_vocabulary(core, vocabulary, vocabulary_threshold)
    pad = core.subword_to_id("<PAD>")
    if not drop_last and (pad == -1 or core.id_to_subword(pad) != "<PAD>"):
        raise click.UsageError("the model was trained without <PAD>: use --drop_last")
    # the C++ pipeline: yttm_encode_file_blocks (host_lines.cpp)
    core.encode_file_blocks(input_path, output, seq_len, core.MODES[mode], bos=bos, eos=eos, reverse=reverse, dropout_prob=dropout_prob, pad_value=pad,
                            tail=2 if drop_last else 0)


@main.command()
@click.option("--model", type=click.Path(exists=True), required=True, help="Path to file with learned model.")
@click.option("--verbose", is_flag=True, help="Add merging rules.")
def vocab(model, verbose):
    """Print list of learned subwords."""
    core = _Core(model)
    core.vocab_cli(verbose)


if __name__ == "__main__":
    main()
