"""Import shim (test infrastructure only) for the reference's `import terminaltables`: the NLQ evaluators only build an
AsciiTable, set column justification and read `.table`."""


class AsciiTable(object):
    def __init__(self, table_data, title=None):
        self.table_data, self.title, self.justify_columns = table_data, title, {}

    @property
    def table(self):
        return "\n".join(" | ".join(str(c).replace("\n", " ") for c in row) for row in self.table_data)
